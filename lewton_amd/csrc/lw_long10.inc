// k_long10: k_long's design -- a workgroup of 16 independent waves per CU, one packet-unit per wave from the entropy records to PCM,
// paced HBM loads, the transform in registers, right halves handed from wave to wave through LDS counters, no barrier after the
// table image is staged -- for blocksize_1 = 10 (n = 1024, what libvorbis writes at 16-22 kHz).  Included at the end of
// lw_kernels_long.hip (it uses that file's packed-arithmetic blocks, register transposes, stores and LDS counter helpers).
//
// A 1024-point channel has 256 complex pairs: 8 per lane on 32 lanes.  So the two channels of a unit sit side by side in the two
// halves of the wave -- lane = 32 c + l: channel c of the unit, lane l of that channel's transform -- instead of one after the
// other as in k_long: a wave holds half of k_long's data (16 residue values and 8 pairs per lane), a 4096-packet batch still is
// 16 waves per CU, and the whole per-channel work (floor values, transform, window, conversion, stores) is issued once for
// both channels.  The transform per half-wave is the block kernel's for L = 32 (layouts B' / C' / D' / E' of lw_fast.hpp, same
// table image LwBlkLayout<32>, tests/short_model.py: the model's two blocks per wave are the two channels here) with a
// conflict-free bit-reverse gather.  What the halves exchange:
//   * loads: lane L of the wave loads float4 number 64 y + L (y = 0, 1) of BOTH residue vectors (two fully coalesced 1 KB
//     requests per vector); the inverse coupling (audio.rs:762-777) runs on these 8 (magnitude, angle) pairs per lane -- every pair
//     once, no lane idle -- and then ONE v_permlane32_swap per dword gives half 0 the magnitude channel's other half and half 1
//     the angle channel's: lane (c, l) ends up with bins 4 (32 x + l) + j, x = 0..3, of channel c, the block kernel's load layout;
//   * floor curves: the two interval tables are built by the whole wave (lanes = posts), every lane then evaluates its own
//     channel's 16 bins.
// EDGE (the stream's short blocks run through k_short<8 / 16>, lw_fast.hpp): a long block with a short slope on either side does
// everything here but the overlap with its short neighbour -- floor, coupling, transform, the full-length overlap on a long side,
// the un-windowed samples past a short slope (audio.rs:1119), the short state -- and leaves the raw edges pa / pb(256 - E .. 255),
// E = blocksize_0 / 4 values per channel, in the edge buffer for k_short, exactly as k_long<EDGE> does for n = 2048.  Without it
// such blocks go to the generic kernels (time-domain blocks exchanged through HBM).
typedef LwBlkLayout<32> Y10;
#define L10_SCR_BYTES 4096u // per wave: 2 x 1 KB interval tables (floor stage), then 2 x 2 KB bit-reverse gather (one per channel)
#define L10_PUB_BYTES 2048u // per wave: published right half [c2][lane] float4
#define L10_LDS_BYTES (Y10::TOTAL + LW_FAST_WAVES * (L10_SCR_BYTES + L10_PUB_BYTES) + 3 * LW_FAST_WAVES * 4)
#define L10_CNT_BASE (Y10::TOTAL + LW_FAST_WAVES * (L10_SCR_BYTES + L10_PUB_BYTES))
#define L10_CNT_PUB(w) (L10_CNT_BASE + 4u * (w))
#define L10_CNT_ACK(w) (L10_CNT_BASE + 4u * (LW_FAST_WAVES + (w)))
#define L10_CNT_LANDED(w) (L10_CNT_BASE + 4u * (2 * LW_FAST_WAVES + (w)))
// tunables (measured on MI355X: tools/ab_cfg.sh, profiles/r05_l10_tuning.txt)
#ifndef L10_FLOOR_FIRST_FROM
#define L10_FLOOR_FIRST_FROM 7 // first wave of a workgroup that builds its floor curves before it requests its residues (>= 4)
#endif
#ifndef L10_IMDCT_PRIO_LATE
#define L10_IMDCT_PRIO_LATE 12 // waves from here on run their transform one priority level up (the last to get data end the launch)
#endif
#ifndef L10_PACE
#define L10_PACE 3             // wave w requests its residues when wave w - L10_PACE has requested its own (16 = no pacing): a wave asks
                               // for half of what a k_long wave does, and three queues side by side keep HBM busy where k_long's single
                               // file does (4096 packets: pace 1 / 2 / 3 / 4 / 8 / 16 = 10.80 / 9.81 / 9.73 / 9.79 / 10.00 / 10.71 us)
#endif
static_assert(Y10::TOTAL / 16u == 832u, "image staging below: 12 waves x 16 bytes per thread + one more row for the first 64");

struct Pref10 {         // what one wave loads from HBM for one item
	float4_t r[2][2];   // residues: lane L holds float4 64 y + L of the unit's first / second channel
	uint32_t fe[2];     // floor-1 post entry of post `lane` of each channel (lanes >= F hold 0)
};

__device__ __forceinline__ void issue_floor_loads10(const LwFastArgs &F, const ItemRegs &it, const LwFastUnit &un, uint32_t lane, Pref10 &p)
{
	const uint16_t *f0 = F.floors + it.floor_off + (uint32_t)un.ch_a * F.fstride;
	p.fe[0] = lane < un.F_a ? (uint32_t)f0[lane] : 0u;
	p.fe[1] = 0u;
	if (un.ch_b >= 0) {
		const uint16_t *f1 = F.floors + it.floor_off + (uint32_t)un.ch_b * F.fstride;
		p.fe[1] = lane < un.F_b ? (uint32_t)f1[lane] : 0u;
	}
}

__device__ __forceinline__ void issue_residue_loads10(const LwFastArgs &F, const ItemRegs &it, const LwFastUnit &un, uint32_t lane, Pref10 &p)
{
	// (non-temporal: read once, see k_long)
	const float4_t *s0 = reinterpret_cast<const float4_t *>(F.residue + it.res_off + (uint32_t)un.ch_a * 512u);
	p.r[0][0] = __builtin_nontemporal_load(&s0[lane]);
	p.r[0][1] = __builtin_nontemporal_load(&s0[64u + lane]);
	if (un.ch_b >= 0) {
		const float4_t *s1 = reinterpret_cast<const float4_t *>(F.residue + it.res_off + (uint32_t)un.ch_b * 512u);
		p.r[1][0] = __builtin_nontemporal_load(&s1[lane]);
		p.r[1][1] = __builtin_nontemporal_load(&s1[64u + lane]);
	} else {
		p.r[1][0] = p.r[1][1] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
	}
}

__device__ __forceinline__ void issue_loads10(const LwFastArgs &F, const ItemRegs &it, const LwFastUnit &un, uint32_t lane, Pref10 &p)
{
	issue_residue_loads10(F, it, un, lane, p);
	issue_floor_loads10(F, it, un, lane, p);
}

__device__ __forceinline__ void dense_offsets10(const LwFastArgs &F, uint32_t item, ItemRegs &it)
{
	it.res_off = item * F.ch * 512u;
	it.floor_off = item * F.ch * F.fstride;
}

// interval table of one channel, lanes = posts (see floor_table: the same entry {dy, c0, 1/adx, w}, the posts' x from this image)
__device__ __forceinline__ bool floor_table10(const char *img, char *sc, uint32_t lane, uint32_t e, uint32_t fslot, uint32_t Fp)
{
	const bool unused = __builtin_amdgcn_readfirstlane(e) == LW_FLOOR_UNUSED;
	const unsigned long long M = __ballot((e & LW_POST_ACTIVE) != 0);
	const unsigned long long lowmask = (2ull << lane) - 1ull;
	const unsigned long long below = M & lowmask, above = M & ~lowmask;
	const int lo = below ? 63 - __builtin_clzll(below) : 0;
	const int hi = above ? __builtin_ctzll(above) : lo;
	const int y = (int)(e & 0xffu);
	const float xs = *reinterpret_cast<const float *>(img + Y10::XSF + 4u * (64u * fslot + lane));
	const int ylo = __builtin_amdgcn_ds_bpermute(lo << 2, y);
	const int yhi = __builtin_amdgcn_ds_bpermute(hi << 2, y);
	const float xlo = __int_as_float(__builtin_amdgcn_ds_bpermute(lo << 2, __float_as_int(xs)));
	const float xhi = __int_as_float(__builtin_amdgcn_ds_bpermute(hi << 2, __float_as_int(xs)));
	const float dy = (float)(yhi - ylo); // 0 when there is no later active post (flat, audio.rs:546-548)
	const float adx = above ? xhi - xlo : 1.0f;
	const bool down = yhi < ylo;
	float4_t ent;
	ent.x = dy;
	ent.y = down ? (0.875f * adx - 0.5f) - xhi * dy : (0.5f - 0.125f * adx) - xlo * dy; // exact
	ent.z = above ? __builtin_amdgcn_rcpf(adx) : 1.0f;
	ent.w = (float)(down ? yhi : ylo) + LW_FLOOR_W0;
	if (lane < Fp)
		*reinterpret_cast<float4_t *>(sc + 16 * lane) = ent;
	return unused;
}

// floor value of bin kf through its interval entry: two fused multiply-adds and a mask (see floor_table)
__device__ __forceinline__ float floor_bin10(float kf, float4_t ent)
{
	const float t = __builtin_fmaf(__builtin_fmaf(kf, ent.x, ent.y), ent.z, ent.w);
	return lds_abs_f32(Y10::INV_DB - 4u + (__float_as_uint(t) & LW_FLOOR_MASK));
}

// this lane's view of its unit: the channel of its half, where that channel's interval table and gather block lie
struct Lane10 {
	uint32_t l;        // lane inside the half (0..31)
	uint32_t tab;      // byte offset of the channel's interval table inside the wave's scratch (0 / 1024)
	uint32_t sidb;     // byte offset of (floor slot, x = 0, l) in the image's static-interval table
	bool unused;       // the channel's floor is unused in this packet (audio.rs:1021-1024)
};

// ---- floor value of the 16 bins 4 (32 x + l) + j of this lane's channel, as ONE software pipeline over the four x (the interval
//      gathers of step x + 2 and the inverse-dB gathers of step x in flight while step x + 1's indices are computed)
//      MUL: spectrum = floor x residue in place (audio.rs:1035-1037); else the floor values themselves (fl)
//      SEL: some channel of the unit has an unused floor (rare): those lanes take 0.0 (0.0 x residue keeps the residue's sign)
template <bool MUL, bool SEL>
__device__ __forceinline__ void floor_values10(const char *img, const char *sc, const Lane10 &ln, float4_t (&X)[4])
{
	const float kf0 = (float)(4 * (int)ln.l);
	uint2_t sid[4];
#pragma unroll
	for (int x = 0; x < 4; x++)
		sid[x] = *reinterpret_cast<const uint2_t *>(img + Y10::SID16 + ln.sidb + 8u * (32u * x));
	const char *tab = sc + ln.tab;
	float4_t ent[2][4];
	float fl[2][4];
#define L10_G(b)                                                       \
	do {                                                               \
		const uint2_t sw = sid[b];                                     \
		ent[(b) & 1][0] = lds4(tab, sw.x & 0xffffu);                   \
		ent[(b) & 1][1] = lds4(tab, sw.x >> 16);                       \
		ent[(b) & 1][2] = lds4(tab, sw.y & 0xffffu);                   \
		ent[(b) & 1][3] = lds4(tab, sw.y >> 16);                       \
	} while (0)
#define L10_XI(b)                                                      \
	do {                                                               \
		_Pragma("unroll") for (int j = 0; j < 4; j++) {                \
			fl[(b) & 1][j] = floor_bin10(kf0 + (float)(128 * (b) + j), ent[(b) & 1][j]); \
			if (SEL)                                                   \
				fl[(b) & 1][j] = ln.unused ? 0.0f : fl[(b) & 1][j];    \
		}                                                              \
	} while (0)
#define L10_M(b)                                                       \
	do {                                                               \
		float4_t &rr = X[b];                                           \
		if (MUL) {                                                     \
			const float2_t lo2 = pk_mul(float2_t{fl[(b) & 1][0], fl[(b) & 1][1]}, float2_t{rr.x, rr.y}); \
			const float2_t hi2 = pk_mul(float2_t{fl[(b) & 1][2], fl[(b) & 1][3]}, float2_t{rr.z, rr.w}); \
			rr = float4_t{lo2.x, lo2.y, hi2.x, hi2.y};                 \
		} else {                                                       \
			rr = float4_t{fl[(b) & 1][0], fl[(b) & 1][1], fl[(b) & 1][2], fl[(b) & 1][3]}; \
		}                                                              \
	} while (0)
	L10_G(0);
	L10_G(1);
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int b = 0; b < 4; b++) {
		L10_XI(b);
		if (b + 2 < 4)
			L10_G(b + 2);
		if (b >= 1)
			L10_M(b - 1);
		__builtin_amdgcn_sched_barrier(0);
	}
	L10_M(3);
#undef L10_G
#undef L10_XI
#undef L10_M
}

// ---- both interval tables (whole wave, lanes = posts), then this lane's view of its own channel
__device__ __forceinline__ Lane10 floor_tables10(const char *img, char *sc, uint32_t lane, const LwFastUnit &un, const uint32_t (&fe)[2], bool two,
		bool &any_unused)
{
	const bool unused0 = floor_table10(img, sc, lane, fe[0], un.floor_a, un.F_a);
	bool unused1 = false;
	if (two)
		unused1 = floor_table10(img, sc + 1024, lane, fe[1], un.floor_b, un.F_b);
	any_unused = unused0 || unused1;
	Lane10 ln;
	const bool second = lane >= 32u && two; // (a single-channel unit: half 1 shadows half 0 and stores nothing)
	ln.l = lane & 31u;
	ln.tab = second ? 1024u : 0u;
	ln.sidb = 8u * ((second ? (uint32_t)un.floor_b : (uint32_t)un.floor_a) * 128u + ln.l);
	ln.unused = second ? unused1 : unused0;
	return ln;
}

// ---- inverse coupling on the load layout (8 pairs per lane, every pair once), then the exchange of halves: X[x] = bins
//      4 (32 x + l) + j of this lane's channel
__device__ __forceinline__ void decouple_swap10(const LwFastUnit &un, Pref10 &pf, float4_t (&X)[4])
{
	if (un.coupled) {
#pragma unroll
		for (int y = 0; y < 2; y++) {
			float m[4] = {pf.r[0][y].x, pf.r[0][y].y, pf.r[0][y].z, pf.r[0][y].w};
			float a[4] = {pf.r[1][y].x, pf.r[1][y].y, pf.r[1][y].z, pf.r[1][y].w};
			decouple4(m[0], a[0], m[1], a[1], m[2], a[2], m[3], a[3]);
			pf.r[0][y] = float4_t{m[0], m[1], m[2], m[3]};
			pf.r[1][y] = float4_t{a[0], a[1], a[2], a[3]};
		}
	}
#pragma unroll
	for (int y = 0; y < 2; y++) {
		// first channel's upper lanes <-> second channel's lower lanes (v_permlane32_swap: lanes 32-63 of its first operand with
		// lanes 0-31 of its second): afterwards the first register holds float4 32 (2y) + l, the second 32 (2y + 1) + l of
		// the lane's own channel
#pragma unroll
		for (int j = 0; j < 4; j++) {
			auto r_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(pf.r[0][y][j]), __float_as_uint(pf.r[1][y][j]), false, false);
			X[2 * y][j] = __uint_as_float(r_[0]);
			X[2 * y + 1][j] = __uint_as_float(r_[1]);
		}
	}
}

// ---- the transform of this lane's channel (imdct.rs:291-659 with n = 1024): spectrum X (load layout) -> R[c2][k] = (pa, pb) at
//      q = 255 - 2m', 254 - 2m', 1 + 2m', 2m' for m' = 2 l + c2: short_imdct<32> on this lane's half of the wave
__device__ __forceinline__ void imdct10(const char *img, char *blk, uint32_t lane, uint32_t l, const float4_t (&X)[4], float2_t (&R)[2][4])
{
	float2_t au[4], al[4], s2[4], l0[2], l1;
#pragma unroll
	for (int x = 0; x < 4; x++) {
		const uint32_t m = 32u * x + l;
		au[x] = lds2(img + Y10::APAIR, 8u * m);          // (A[2m], A[2m+1])
		al[x] = lds2(img + Y10::APAIR, 8u * (255u - m)); // (A[510-2m], A[511-2m])
		s2[x] = lds2(img + Y10::TW_S2, 8u * m);
	}
	l0[0] = lds2(img + Y10::TW_L0, 8u * l);
	l0[1] = lds2(img + Y10::TW_L0, 8u * (32u + l));
	l1 = lds2(img + Y10::TW_L1, 8u * l);
	float2_t Q[8], U[4];
	step1x2(X[0], au[0], al[0], X[1], au[1], al[1], U[0], Q[0], U[1], Q[1]);
	step1x2(X[2], au[2], al[2], X[3], au[3], al[3], U[2], Q[2], U[3], Q[3]);
	const uint32_t mirror = (lane ^ 31u) << 2;
#pragma unroll
	for (int x = 0; x < 4; x++) { // pair 255 - m lives on the mirror lane of the half
		Q[7 - x].x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(U[x].x)));
		Q[7 - x].y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(U[x].y)));
	}
	bfly2x4(Q[4], Q[0], s2[0], Q[5], Q[1], s2[1], Q[6], Q[2], s2[2], Q[7], Q[3], s2[3]); // step 2 (imdct.rs:385-430)
	bfly2x4(Q[2], Q[0], l0[0], Q[6], Q[4], l0[0], Q[3], Q[1], l0[1], Q[7], Q[5], l0[1]); // l = 0
	bfly2x4(Q[1], Q[0], l1, Q[3], Q[2], l1, Q[5], Q[4], l1, Q[7], Q[6], l1);             // l = 1
	blk_t2<32>(Q);                                                                       // register bits 1, 0 <-> lane bits 4, 3
	{
		const uint32_t lo3 = l & 7u;
		const float2_t c2a = lds2(img + Y10::TW_C2, 8u * lo3), c2b = lds2(img + Y10::TW_C2, 8u * (8u + lo3));
		const float2_t c3 = lds2(img + Y10::TW_C3, 8u * lo3);
		bfly2x4(Q[2], Q[0], c2a, Q[6], Q[4], c2a, Q[3], Q[1], c2b, Q[7], Q[5], c2b);     // l = 2 (imdct.rs:454-477)
		bfly2x4(Q[1], Q[0], c3, Q[3], Q[2], c3, Q[5], Q[4], c3, Q[7], Q[6], c3);         // l = 3
	}
	t3_inreg(Q);                                                                         // -> D': register = p[2:0]
	const float a2s = *reinterpret_cast<const float *>(img + Y10::A2);
	stage_d_block(float2_t{a2s, a2s}, Q);                                                // imdct.rs:234-288
	// bit-reverse gather through the channel's 2 KB block, conflict-free slots (blk_slot<32>, lw_kernels_long.hip)
	const uint32_t hi = ((l >> 2) & 1u) << 4 | ((l >> 4) & 1u) << 3 | ((l >> 3) & 1u) << 2 | ((l >> 1) & 1u) << 1 | (l & 1u); // (p7 .. p3) = lane bits (2, 4, 3, 1, 0)
	const uint32_t wbase = 8u * blk_slot<32>(0, 8u * hi);
#pragma unroll
	for (int zz = 0; zz < 8; zz++)
		*reinterpret_cast<float2_t *>(blk + (wbase ^ (8u * blk_slot<32>(0, zz)))) = Q[zz];
	lds_fence();
	const uint32_t rbase = 8u * blk_slot<32>(0, 2u * (__builtin_bitreverse32(2u * l) >> 26)); // pair 2v, v = rev6(2 l)
#pragma unroll
	for (int c2 = 0; c2 < 2; c2++) { // bit-reverse gather (imdct.rs:490-528), step 7 (:533-580), step 8 (:589-658)
		const uint32_t kc = (uint32_t)c2 << 6;
		const float2_t pq = lds2(blk, rbase ^ (8u * blk_slot<32>(0, kc))), pqh = lds2(blk, rbase ^ (8u * blk_slot<32>(0, kc ^ 128u)));
		const float2_t ph = lds2(blk, rbase ^ (8u * blk_slot<32>(0, kc ^ 127u))), pf = lds2(blk, rbase ^ (8u * blk_slot<32>(0, kc ^ 255u)));
		const float4_t Cq = lds4(img + Y10::C4, 16u * (32u * c2 + l));
		const float4_t Bl = lds4(img + Y10::B_LO, 16u * (32u * c2 + l)), Bh = lds4(img + Y10::B_HI, 16u * (32u * c2 + l));
		step78_block(pf, pq, ph, pqh, Cq, Bl, Bh, R[c2]);
	}
	lds_fence();
}

// ---- interleaved i16 of a 2-channel stream decoded as ONE unit (InterleavedSamples<i16>, samples.rs:48-78; `read_dec_packet_itl`): the
//      two halves of the wave hold the two channels' samples of the same positions.  Window, overlap-add and conversion as in
//      short_ola_store; then, per group of four positions, ONE v_permlane32_swap brings the first channel's and the second channel's
//      packed pairs to one lane -- positions +2, +3 to the lower half, +0, +1 to the upper -- which stores two (L, R) frames as 8 bytes
//      (the generic form: sixteen 2-byte stores per lane at stride ch)
__device__ __forceinline__ void ola_store_itl2_10(const char *img, uint32_t lane, uint32_t l, void *out, uint32_t out_off, bool first_is_ch0,
		const float2_t (&Rc)[2][4], const PrevHalf &h)
{
	float2_t O[2][4];
#pragma unroll
	for (int c2 = 0; c2 < 2; c2++) {
		const float4_t w0 = lds4(img + Y10::WIN, 32u * (32u * c2 + l));
		const float4_t w1 = lds4(img + Y10::WIN, 32u * (32u * c2 + l) + 16u);
		ola_block<true>(Rc[c2], h.pp[c2][0], h.pp[c2][1], w0, w1, O[c2]);
	}
	const uint32_t pos[4] = {4u * l, 252u - 4u * l, 256u + 4u * l, 508u - 4u * l};
	const float v[4][4] = {{O[0][3].x, O[0][2].x, O[1][3].x, O[1][2].x}, {O[1][1].x, O[1][0].x, O[0][1].x, O[0][0].x},
		{O[0][0].y, O[0][1].y, O[1][0].y, O[1][1].y}, {O[1][2].y, O[1][3].y, O[0][2].y, O[0][3].y}};
	int16_t *o = reinterpret_cast<int16_t *>(out) + out_off;
	const uint32_t sub = lane >= 32u ? 0u : 2u; // which two of the group's four positions this lane stores
#pragma unroll
	for (int q = 0; q < 4; q++) {
		typedef short short2_t __attribute__((ext_vector_type(2)));
		union {
			short2_t s;
			uint32_t u;
		} a, b;
		a.s = __builtin_amdgcn_cvt_pk_i16((int)v[q][0], (int)v[q][1]); // samples.rs:92-103 (x 32768 in ola_block; saturating conversions)
		b.s = __builtin_amdgcn_cvt_pk_i16((int)v[q][2], (int)v[q][3]);
		// lanes 32-63 of b <-> lanes 0-31 of a: afterwards X = the first channel's pair, Y = the second channel's, in both halves
		auto r_ = __builtin_amdgcn_permlane32_swap(b.u, a.u, false, false);
		const uint32_t X = r_[0], Y = r_[1];
		const uint32_t c0 = first_is_ch0 ? X : Y, c1 = first_is_ch0 ? Y : X;
		const uint32_t d0 = __builtin_amdgcn_perm(c1, c0, 0x05040100u); // (ch0[p], ch1[p])
		const uint32_t d1 = __builtin_amdgcn_perm(c1, c0, 0x07060302u); // (ch0[p+1], ch1[p+1])
		store_pcm8(o + 2u * (pos[q] + sub), d0, d1);
	}
}

// ---- the same for interleaved f32 (InterleavedSamples<f32>, samples.rs:48-78, :86-90): per group of four positions, two
//      v_permlane32_swap bring both channels' samples of two positions -- +2, +3 to the lower half, +0, +1 to the upper -- to one
//      lane, which stores the two (L, R) frames as 16 bytes: four 16-byte stores per lane, as for f32 planar
__device__ __forceinline__ void ola_store_itl2_10_f32(const char *img, uint32_t lane, uint32_t l, void *out, uint32_t out_off,
		bool first_is_ch0, const float2_t (&Rc)[2][4], const PrevHalf &h)
{
	float2_t O[2][4];
#pragma unroll
	for (int c2 = 0; c2 < 2; c2++) {
		const float4_t w0 = lds4(img + Y10::WIN, 32u * (32u * c2 + l));
		const float4_t w1 = lds4(img + Y10::WIN, 32u * (32u * c2 + l) + 16u);
		ola_block<false>(Rc[c2], h.pp[c2][0], h.pp[c2][1], w0, w1, O[c2]);
	}
	const uint32_t pos[4] = {4u * l, 252u - 4u * l, 256u + 4u * l, 508u - 4u * l};
	const float v[4][4] = {{O[0][3].x, O[0][2].x, O[1][3].x, O[1][2].x}, {O[1][1].x, O[1][0].x, O[0][1].x, O[0][0].x},
		{O[0][0].y, O[0][1].y, O[1][0].y, O[1][1].y}, {O[1][2].y, O[1][3].y, O[0][2].y, O[0][3].y}};
	float *o = reinterpret_cast<float *>(out) + out_off;
	const uint32_t sub = lane >= 32u ? 0u : 2u; // which two of the group's four positions this lane stores
#pragma unroll
	for (int q = 0; q < 4; q++) {
		// lanes 32-63 of (v2, v3) <-> lanes 0-31 of (v0, v1): afterwards X = the first channel's two samples, Y = the second's
		auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[q][2]), __float_as_uint(v[q][0]), false, false);
		auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[q][3]), __float_as_uint(v[q][1]), false, false);
		const float x0 = __uint_as_float(r0[0]), x1 = __uint_as_float(r1[0]), y0 = __uint_as_float(r0[1]), y1 = __uint_as_float(r1[1]);
		store16_wt(o + 2u * (pos[q] + sub), first_is_ch0 ? float4_t{x0, y0, x1, y1} : float4_t{y0, x0, y1, x1});
	}
}

// raw halves at this lane's q positions (see Half8): lo = q in [4l, 4l+4), hi = q in [252 - 4l, 256 - 4l)
#define L10_PB_LO(R_) float4_t{R_[0][3].y, R_[0][2].y, R_[1][3].y, R_[1][2].y}
#define L10_PB_HI(R_) float4_t{R_[1][1].y, R_[1][0].y, R_[0][1].y, R_[0][0].y}
#define L10_PA_LO(R_) float4_t{R_[0][3].x, R_[0][2].x, R_[1][3].x, R_[1][2].x}
#define L10_PA_HI(R_) float4_t{R_[1][1].x, R_[1][0].x, R_[0][1].x, R_[0][0].x}

// ---- k_mix10: a mixed short / long batch of a blocksize_1 = 10 stream in ONE launch (what k_mix is to k_long): the last
// LW_MIX_SHORT_WAVES waves of every workgroup of k_long10<EDGE>'s launch run k_short<MIXL>'s work (one channel per wave, areas of their
// own behind the long blocks' LDS, the short blocks' image staged with the long blocks'); a long block's wave sets a flag in HBM
// behind each raw edge it has written through, a short block's wave waits for the flags of its two edges only when it reaches its
// overlap-add.  The whole grid is resident (one workgroup per CU, lw_mix10_applicable), so nobody waits for a wave that cannot run;
// a wave whose flags never come raises the batch's device error word instead of storing samples (lw_short_body.inc).
#define L10_MIX_IMG_OFF ((L10_LDS_BYTES + 15u) & ~15u) // the short blocks' image behind k_long10's own LDS, their waves' areas behind it
template <int L>
struct L10Mix {
	static constexpr uint32_t AREAS = L10_MIX_IMG_OFF + LwBlkLayout<L>::TOTAL;
	static constexpr uint32_t LDS_BYTES = AREAS + LW_MIX_SHORT_WAVES * LwBlkWave<L, true>::BYTES;
	static constexpr uint32_t ROWS = LwBlkLayout<L>::TOTAL / 16u; // 16-byte rows of the image: staged by the 256 threads of the last four waves
};
static_assert(L10Mix<8>::LDS_BYTES <= 160u * 1024u && L10Mix<16>::LDS_BYTES <= 160u * 1024u, "k_mix10's LDS fits a CU");
static_assert(L10Mix<8>::ROWS <= 512u && L10Mix<16>::ROWS <= 512u, "two rows per staging thread");

template <int FMT, int L>
__device__ __forceinline__ void mix10_short_role(const LwShortArgs &F, const LwMixArgs &M, char *smem_dyn, uint32_t wave, uint32_t lane)
{
	uint32_t *const edge_flags = M.flags, *const mix_err = M.err;
	const uint32_t mix_spin = M.spin;
	const uint32_t i = wave - (LW_FAST_WAVES - LW_MIX_SHORT_WAVES);
	const uint32_t wid = blockIdx.x * LW_MIX_SHORT_WAVES + i; // this wave's (task, unit half)
	if (wid >= F.n_waves)
		return;
	char *const smem_all = smem_dyn + L10_MIX_IMG_OFF;
	char *const smem = smem_dyn + L10Mix<L>::AREAS + i * LwBlkWave<L, true>::BYTES;
	constexpr bool STAGE = false;
	if (__builtin_amdgcn_readfirstlane((uint32_t)F.units[wid % F.n_units].slot) == 0u) {
		constexpr int ONLY = 0;
#include "lw_short_body.inc"
	} else {
		constexpr int ONLY = 1;
#include "lw_short_body.inc"
	}
}

// MIXL: 0, or the lanes per short block (8 / 16) of the short role (k_mix10; FSp / Mp valid)
template <int FMT, bool RIGHT_ONLY, bool EDGE, int MIXL>
__device__ __forceinline__ void long10_body(const LwFastArgs &F, const LwShortArgs *FSp, const LwMixArgs *Mp)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const uint32_t lane_id = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t n_units = F.n_units, per_round = F.per_round, rounds = F.rounds;
	LwFastUnit un;
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const unsigned long long __attribute__((address_space(4))) *ka_ptr;
	const unsigned long long unit_word = ((ka_ptr)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(LwFastArgs, waves) / 8 + wave];
#else
	const unsigned long long unit_word = 0;
#endif
	// ONE batch of kernel-argument loads behind one wait (see lw_long_body.inc)
	asm volatile("" ::"s"(F.residue), "s"(F.floors), "s"(F.n_items), "s"(n_units), "s"(per_round), "s"(rounds), "s"(F.dense),
			"s"(F.late_from), "s"(F.ch), "s"(F.fstride), "s"(F.image), "s"(unit_word));
	__builtin_memcpy(&un, &unit_word, 8);
	const uint32_t slot = un.slot, uidx = wave - slot * n_units; // packet slot of the round, unit of the packet
	const bool active = slot < per_round;
	const uint32_t item0 = blockIdx.x * per_round * rounds + slot; // item of round j = item0 + j * per_round
	const bool two = un.ch_b >= 0;
	const bool late = !RIGHT_ONLY && wave >= (F.late_from > LW_PRE_WAVES ? F.late_from : (uint32_t)LW_PRE_WAVES);

	// ---- round 0: table image (L2-resident) and residues / floors (HBM); early waves queue their HBM loads first
	ItemRegs it{};
	Pref10 pf{};
	bool valid = active && item0 < F.n_items;
	if (valid) {
		if (F.dense)
			dense_offsets10(F, item0, it);
		else
			it = load_item(F.items, item0);
	}
	const bool floor_first = late && F.late_from < LW_FAST_WAVES && wave >= L10_FLOOR_FIRST_FROM;
	if (wave < 4) {
		if (valid && !late)
			issue_loads10(F, it, un, lane_id, pf);
	} else {
		const uint32_t t = threadIdx.x - 256u;
		const uint4 *src = reinterpret_cast<const uint4 *>(F.image) + t;
		uint4 *dst = reinterpret_cast<uint4 *>(smem) + t;
		const uint4 v0 = src[0];
		uint4 v1 = make_uint4(0, 0, 0, 0);
		if (t < 64u)
			v1 = src[768];
		// (k_mix10: the short blocks' image is requested in the same round trip, by the threads of the last four waves ...)
		constexpr uint32_t SROWS = MIXL ? L10Mix<MIXL ? MIXL : 8>::ROWS : 0u;
		const bool s_on = MIXL && t >= 512u, s_two = s_on && t - 512u + 256u < SROWS;
		const uint4 *s_src = reinterpret_cast<const uint4 *>(MIXL ? FSp->image : F.image) + (s_on ? t - 512u : 0u);
		uint4 s_v0 = make_uint4(0, 0, 0, 0), s_v1 = s_v0;
		if (s_on && t - 512u < SROWS)
			s_v0 = s_src[0];
		if (s_two)
			s_v1 = s_src[256];
		if (t < 3 * LW_FAST_WAVES)
			lds_store_u32(L10_CNT_BASE + 4u * t, 0u);
		dst[0] = v0;
		if (t < 64u)
			dst[768] = v1;
		if (MIXL) { // (... and stored in front of the same barrier)
			uint4 *s_dst = reinterpret_cast<uint4 *>(smem + L10_MIX_IMG_OFF) + (s_on ? t - 512u : 0u);
			if (s_on && t - 512u < SROWS)
				s_dst[0] = s_v0;
			if (s_two)
				s_dst[256] = s_v1;
		}
		lds_fence();
		if (valid && !late)
			issue_loads10(F, it, un, lane_id, pf);
		if (valid && floor_first)
			issue_floor_loads10(F, it, un, lane_id, pf);
	}
	__syncthreads();
	if (MIXL && wave >= LW_FAST_WAVES - LW_MIX_SHORT_WAVES) { // k_mix10: the workgroup's last waves leave for the short blocks here
		mix10_short_role<FMT, MIXL ? MIXL : 8>(*FSp, *Mp, smem, wave, lane_id);
		return;
	}
	const char *img = smem;
	char *sc = smem + Y10::TOTAL + wave * L10_SCR_BYTES;
	char *pub0 = smem + Y10::TOTAL + LW_FAST_WAVES * L10_SCR_BYTES; // [wave][L10_PUB_BYTES]
	char *pub = pub0 + wave * L10_PUB_BYTES;
	const bool paced = !RIGHT_ONLY && F.late_from < LW_FAST_WAVES;
	uint32_t lane0 = lane_id;
	asm volatile("" : "+v"(lane0)); // (laundered: see lw_long_body.inc)
	float4_t X[4]; // spectrum of this lane's channel, load layout
	if (valid && floor_first) {
		// floor curves while the wave waits for its turn in the residue queue: when the residues land, only the inverse coupling,
		// the exchange of halves and one multiply per bin are left
		float4_t fl[4];
		bool any_unused;
		__builtin_amdgcn_s_setprio(LW_PRIO_FLOOR);
		const Lane10 ln = floor_tables10(img, sc, lane0, un, pf.fe, two, any_unused);
		lds_fence();
		if (any_unused)
			floor_values10<false, true>(img, sc, ln, fl);
		else
			floor_values10<false, false>(img, sc, ln, fl);
		lds_fence();
		__builtin_amdgcn_s_setprio(LW_PRIO_PACE);
		lds_wait_ge(L10_CNT_LANDED(wave - F.late_from), 1u);
		issue_residue_loads10(F, it, un, lane_id, pf);
		if (wave + F.late_from < LW_FAST_WAVES) {
			asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW_PACE_VMCNT) : "memory");
			lds_store_u32(L10_CNT_LANDED(wave), 1u);
		}
		if (F.dense)
			it = load_item(F.items, item0); // the rest of the item; its latency hides behind the residues'
		__builtin_amdgcn_s_setprio(LW_PRIO_READY);
		decouple_swap10(un, pf, X);
#pragma unroll
		for (int x = 0; x < 4; x++) {
			const float2_t lo2 = pk_mul(float2_t{fl[x].x, fl[x].y}, float2_t{X[x].x, X[x].y});
			const float2_t hi2 = pk_mul(float2_t{fl[x].z, fl[x].w}, float2_t{X[x].z, X[x].w});
			X[x] = float4_t{lo2.x, lo2.y, hi2.x, hi2.y};
		}
		__builtin_amdgcn_s_setprio(0);
	} else {
		if (paced) {
			__builtin_amdgcn_s_setprio(LW_PRIO_PACE);
			if (late) {
				lds_wait_ge(L10_CNT_LANDED(wave - F.late_from), 1u);
				if (valid)
					issue_loads10(F, it, un, lane_id, pf);
			}
			if (wave + F.late_from < LW_FAST_WAVES) {
				asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW_PACE_VMCNT) : "memory");
				lds_store_u32(L10_CNT_LANDED(wave), 1u);
			}
			__builtin_amdgcn_s_setprio(0);
		}
		if (valid && F.dense)
			it = load_item(F.items, item0);
		if (valid) {
			bool any_unused;
			__builtin_amdgcn_s_setprio(LW_PRIO_FLOOR);
			const Lane10 ln = floor_tables10(img, sc, lane0, un, pf.fe, two, any_unused);
			lds_fence();
			decouple_swap10(un, pf, X);
			if (any_unused)
				floor_values10<true, true>(img, sc, ln, X);
			else
				floor_values10<true, false>(img, sc, ln, X);
			lds_fence();
			__builtin_amdgcn_s_setprio(0);
		}
	}
	uint32_t n_pub_used = 0; // hand-overs published by this wave (only those a successor reads are published)
	uint32_t n_got = 0;      // hand-overs consumed from the predecessor wave
	const uint32_t wprev = slot != 0 ? wave - n_units : (per_round - 1) * n_units + uidx;

	for (uint32_t j = 0; j < rounds; j++) {
		uint32_t lane = lane_id;
		asm volatile("" : "+v"(lane));
		const uint32_t l = lane & 31u;
		const bool second = lane >= 32u;
		const bool mine = !second || two;                       // this half holds a channel of the unit
		const uint32_t chn = (uint32_t)(second && two ? un.ch_b : un.ch_a);
		float2_t R[2][4]; // [c2][k] = (pa, pb) at q_k(m' = 2 l + c2) of this lane's channel: un-windowed left / right halves
		const uint32_t item_n = item0 + (j + 1) * per_round;
		const bool valid_n = active && j + 1 < rounds && item_n < F.n_items;
		ItemRegs itn{};
		if (valid_n && !F.dense)
			itn = load_item(F.items, item_n);
		if (valid) {
			// (k_mix10: the long blocks' waves share their SIMDs with short blocks' waves that will wait for them: one level up)
			if (wave >= L10_IMDCT_PRIO_LATE)
				__builtin_amdgcn_s_setprio(LW_PRIO_IMDCT + 1 + (MIXL ? 1 : 0));
			else
				__builtin_amdgcn_s_setprio(LW_PRIO_IMDCT + (MIXL ? 1 : 0));
			imdct10(img, sc + (second ? 2048u : 0u), lane, l, X, R);
		}
		if (valid) {
			if (RIGHT_ONLY) {
				if (mine) {
					float *dst = F.halo + ((size_t)it.halo_out * F.ch + chn) * 256u;
					*reinterpret_cast<float4_t *>(dst + 4u * l) = L10_PB_LO(R);
					*reinterpret_cast<float4_t *>(dst + 252u - 4u * l) = L10_PB_HI(R);
				}
			} else {
				__builtin_amdgcn_s_setprio(LW_PRIO_FINISH); // finish: hand-over, overlap-add, stores
				// EDGE: geometry of a long block with a short slope on the left (the window starts at 256 - E, the first 2 E samples
				// are k_short's) and / or on the right (samples up to 768 - E, a right part of 2 E values); E = blocksize_0 / 4
				const bool edge_l = EDGE && (it.flags & LW_IF_EDGE_L), edge_r = EDGE && (it.flags & LW_IF_EDGE_R);
				const uint32_t E = EDGE ? F.edge_n : 0u;
				const uint32_t e_ls = edge_l ? 256u - E : 0u, e_m = EDGE ? (edge_r ? 768u - E : 512u) - e_ls : 512u;
				if (MIXL && (edge_l || edge_r)) {
					// k_mix10: short blocks' waves of this very launch wait for the raw edges -- out with them first, written through, and
					// the flags behind them (the edge stores further down are skipped)
					if (mine && l < E / 4u) {
						float *edge = F.edge + ((size_t)it.pkt * 2u * F.ch + chn) * E;
						if (edge_l)
							store16_wt(edge + (E - 4u) - 4u * l, L10_PA_HI(R));
						if (edge_r)
							store16_wt(edge + (size_t)F.ch * E + (E - 4u) - 4u * l, L10_PB_HI(R));
					}
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
					if (mine && l == 0 && !Mp->drop_flags) { // (drop_flags: test hook, a producer that never signals)
						uint32_t *fl = Mp->flags + ((size_t)it.pkt * 2u) * F.ch + chn;
						if (edge_l)
							__hip_atomic_store(fl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						if (edge_r)
							__hip_atomic_store(fl + F.ch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					}
				}
				// ---- publish my right half: wait until the previous one has been read, write, bump the counter
				if (it.flags & LW_IF_NEXT_LDS) {
					lds_wait_ge(L10_CNT_ACK(wave), n_pub_used);
#pragma unroll
					for (int c2 = 0; c2 < 2; c2++)
						*reinterpret_cast<float4_t *>(pub + 16u * (64u * c2 + lane)) =
							float4_t{R[c2][0].y, R[c2][1].y, R[c2][2].y, R[c2][3].y};
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					n_pub_used++;
					lds_store_u32(L10_CNT_PUB(wave), n_pub_used);
				}
				// ---- the previous packet's right half: from my predecessor wave through LDS, or (chunk starts) from the stream's
				//      state slot / the halo buffer / a generic predecessor's time-domain block; window, overlap-add, conversion, stores
				if (it.src_kind != LW_SRC_NONE) {
					PrevHalf ph;
					if (it.src_kind == LW_SRC_LDS) {
						++n_got;
						lds_wait_ge(L10_CNT_PUB(wprev), n_got);
						const char *src = pub0 + wprev * L10_PUB_BYTES;
#pragma unroll
						for (int c2 = 0; c2 < 2; c2++) {
							const float4_t v = *reinterpret_cast<const float4_t *>(src + 16u * (64u * c2 + lane));
							ph.pp[c2][0] = float2_t{v.x, v.y};
							ph.pp[c2][1] = float2_t{v.z, v.w};
						}
					} else {
						const float *g;
						uint32_t cstride;
						if (it.src_kind == LW_SRC_STATE) {
							const uint32_t pin = (it.flags & LW_RF_PARITY_IN) ? 1u : 0u;
							g = F.state + ((size_t)it.src_arg * 2 + pin) * F.state_stride;
							cstride = F.state_chan_stride;
						} else if (it.src_kind == LW_SRC_HALO) {
							g = F.halo + (size_t)it.src_arg * F.ch * 256u;
							cstride = 256u;
						} else { // LW_SRC_TD: second half of the predecessor's [ch][1024] time-domain block
							g = F.td + (size_t)it.src_arg + 512u;
							cstride = 1024u;
						}
						prev_from_half8(load_half8<32>(g + chn * cstride, l), ph);
					}
					if (FMT == LW_OUT_I16_INTERLEAVED && two && F.ch == 2u) {
						ola_store_itl2_10(img, lane, l, F.out, it.out_off, un.ch_a == 0, R, ph); // (both halves: a frame needs both channels)
					} else if (FMT == LW_OUT_F32_INTERLEAVED && two && F.ch == 2u) {
						ola_store_itl2_10_f32(img, lane, l, F.out, it.out_off, un.ch_a == 0, R, ph);
					} else if (mine) {
						const uint32_t e0 = lw_out_itl(FMT) ? it.out_off + chn : it.out_off + chn * e_m;
						short_ola_store<FMT, 32>(img, l, F.out, e0, lw_out_itl(FMT) ? F.ch : 1u, R, ph);
					}
					if (it.src_kind == LW_SRC_LDS) {
						asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
						lds_store_u32(L10_CNT_ACK(wprev), n_got);
					}
				}
				if (EDGE && (edge_l || edge_r) && mine) {
					// ---- short slopes: the un-windowed samples past them, the raw edges for k_short, the short state
					const bool inner = l >= E / 4u; // this lane's q in [252 - 4 l, +4) lies below 256 - E
					const bool sound = !(it.flags & LW_IF_SILENT); // (the first packet of a stream yields no samples at all)
					float *edge = F.edge + ((size_t)it.pkt * 2u * F.ch + chn) * E;
					if (edge_l) {
						// cur[511 - q] = -pa(q) for q < 256 - E (imdct.rs:589-658): positions 256 + E .. 511
						const float4_t lo = L10_PA_LO(R), hi = L10_PA_HI(R);
						store_quad<FMT>(F, (int)chn, it.out_off, e_m, 508u - 4u * l - e_ls, float4_t{-lo.w, -lo.z, -lo.y, -lo.x}, sound);
						store_quad<FMT>(F, (int)chn, it.out_off, e_m, 256u + 4u * l - e_ls, float4_t{-hi.w, -hi.z, -hi.y, -hi.x}, sound && inner);
						if (!inner && !MIXL) // raw left edge pa(256 - E + i), i = E - 4 - 4 l ..
							store16_wt(edge + (E - 4u) - 4u * l, hi);
					}
					if (edge_r) {
						// cur[512 + q] = pb(q) for q < 256 - E: positions 512 .. 767 - E
						const float4_t lo = L10_PB_LO(R), hi = L10_PB_HI(R);
						store_quad<FMT>(F, (int)chn, it.out_off, e_m, 512u + 4u * l - e_ls, lo, sound);
						store_quad<FMT>(F, (int)chn, it.out_off, e_m, 764u - 4u * l - e_ls, hi, sound && inner);
						if (!inner) { // raw right part cur[768 - E .. 768 + E): pb(256 - E + i), then mirrored
							if (!MIXL)
								store16_wt(edge + (size_t)F.ch * E + (E - 4u) - 4u * l, hi);
							if (it.state_out >= 0) {
								float *dst = F.state + ((size_t)it.state_out * 2 + ((it.flags & LW_RF_PARITY_OUT) ? 1u : 0u)) * F.state_stride +
									chn * F.state_chan_stride;
								store16_wt(dst + (E - 4u) - 4u * l, hi);
								store16_wt(dst + E + 4u * l, float4_t{hi.w, hi.z, hi.y, hi.x});
							}
						}
					}
				}
				// ---- raw right half to the stream's state slot and / or to the td block a generic successor reads
				if (mine && it.state_out >= 0 && !edge_r) {
					const uint32_t pout = (it.flags & LW_RF_PARITY_OUT) ? 1u : 0u;
					short_store_right<32>(F.state + ((size_t)it.state_out * 2 + pout) * F.state_stride + chn * F.state_chan_stride, l, R);
				}
				if (mine && (it.flags & LW_RF_WRITE_TD))
					short_store_right<32>(F.td + 2u * (size_t)it.res_off + chn * 1024u + 512u, l, R);
				if (EDGE && mine && (it.flags & LW_IF_TDONLY)) {
					// a block whose window / overlap-add k_ola_generic does (short slopes without an edge form): the un-windowed left
					// half too -- cur[q] = pa(q), cur[511 - q] = -pa(q) (imdct.rs:589-658)
					float *dst = F.td + 2u * (size_t)it.res_off + chn * 1024u;
					const float4_t lo = L10_PA_LO(R), hi = L10_PA_HI(R);
					store16_wt(dst + 4u * l, lo);
					store16_wt(dst + 252u - 4u * l, hi);
					store16_wt(dst + 256u + 4u * l, float4_t{-hi.w, -hi.z, -hi.y, -hi.x});
					store16_wt(dst + 508u - 4u * l, float4_t{-lo.w, -lo.z, -lo.y, -lo.x});
				}
			}
		}
		__builtin_amdgcn_s_setprio(0);
		// ---- HBM loads of the next round, and its spectrum
		if (valid_n) {
			if (F.dense) {
				dense_offsets10(F, item_n, itn);
				issue_loads10(F, itn, un, lane, pf);
				itn = load_item(F.items, item_n);
			} else {
				issue_loads10(F, itn, un, lane, pf);
			}
			bool any_unused;
			__builtin_amdgcn_s_setprio(LW_PRIO_FLOOR);
			const Lane10 ln = floor_tables10(img, sc, lane, un, pf.fe, two, any_unused);
			lds_fence();
			decouple_swap10(un, pf, X);
			if (any_unused)
				floor_values10<true, true>(img, sc, ln, X);
			else
				floor_values10<true, false>(img, sc, ln, X);
			lds_fence();
			__builtin_amdgcn_s_setprio(0);
		}
		it = itn;
		valid = valid_n;
	}
}

template <int FMT, bool RIGHT_ONLY, bool EDGE = false>
__global__ void __launch_bounds__(LW_WG) k_long10(LwFastArgs F)
{
	long10_body<FMT, RIGHT_ONLY, EDGE, 0>(F, nullptr, nullptr);
}

template <int FMT, int L>
__global__ void __launch_bounds__(LW_WG) k_mix10(LwFastArgs F, LwShortArgs FS, LwMixArgs M)
{
	long10_body<FMT, false, true, L>(F, &FS, &M);
}

// per-device attributes, the halo pre-pass, and the kernel arguments + grid of the main pass (also the long role of k_mix10)
static hipError_t long10_prepare(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, hipStream_t st, LwFastArgs &F,
		dim3 &grid);

hipError_t lw_launch_long10(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, int fmt, hipStream_t st)
{
	LwFastArgs F{};
	dim3 grid(0);
	const hipError_t pe = long10_prepare(T, B, L, out, st, F, grid);
	if (pe != hipSuccess || !L.n_items)
		return pe;
	const dim3 block(LW_WG);
	const size_t lds = L10_LDS_BYTES;
	if (L.edge_mode || L.has_tdonly) // (chosen per batch: an all-(1,1) batch keeps the plain kernel)
		return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_long10<f.value, false, true>, grid, block, lds, st, F); });
	return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_long10<f.value, false>, grid, block, lds, st, F); });
}

// ---- k_mix10: can the two launches of a mixed batch run as one, and the launch itself (see lw_mix_applicable / lw_launch_mix)
bool lw_mix10_applicable(const LwFastLaunch &LL, const LwShortLaunch &LS, int n_cus)
{
	if (!LL.n_items || !LL.edge_mode || LL.rounds != 1 || !LS.n_tasks || (LS.lanes != 8 && LS.lanes != 16) || LS.passes > 1)
		return false;
	if ((size_t)LS.n_tasks * LS.n_units > LW_SHORT_SPLIT_BELOW || 2 * LS.n_units > LW_FAST_WAVES) // (short_prepare splits the pairs then)
		return false;
	for (uint32_t u = 0; u < LS.n_units; u++)
		if (LS.units[u].ch_b < 0)
			return false;
	if (LL.per_round * LL.n_units > LW_FAST_WAVES - LW_MIX_SHORT_WAVES) // the long blocks' waves: 0 .. 11
		return false;
	const size_t n_wg = (LL.n_items + LL.per_round - 1) / LL.per_round;
	return n_wg <= (size_t)std::max(1, n_cus) && (size_t)LS.n_tasks * LS.n_units * 2 <= n_wg * LW_MIX_SHORT_WAVES;
}

hipError_t lw_launch_mix10(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &LL, const LwShortLaunch &LS, uint32_t *d_flags,
		uint32_t *d_err, uint32_t spin, bool drop_flags, void *out, int fmt, hipStream_t st)
{
	LwFastArgs F{};
	dim3 grid(0);
	const hipError_t pe = long10_prepare(T, B, LL, out, st, F, grid);
	if (pe != hipSuccess)
		return pe;
	const dim3 block(LW_WG);
	return mix_launch(T, B, LS, d_flags, d_err, spin, drop_flags, out, st, [&](LwShortArgs &FS, LwMixArgs &M) {
		const size_t lds8 = L10Mix<8>::LDS_BYTES, lds16 = L10Mix<16>::LDS_BYTES;
		if (LS.lanes == 8)
			return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_mix10<f.value, 8>, grid, block, lds8, st, F, FS, M); });
		return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_mix10<f.value, 16>, grid, block, lds16, st, F, FS, M); });
	});
}

static hipError_t long10_prepare(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, hipStream_t st, LwFastArgs &F,
		dim3 &grid)
{
	F.image = L.d_image;
	F.residue = B.residue;
	F.floors = B.floors;
	F.state = B.state;
	F.td = B.td;
	F.ch = T.ch;
	F.fstride = T.fstride;
	F.state_stride = T.state_stride;
	F.state_chan_stride = T.state_chan_stride;
	F.n_units = L.n_units;
	F.halo = L.d_halo;
	F.edge = L.d_edge;
	F.edge_n = L.edge_n;
	F.out = out;
	for (uint32_t w = 0; w < LW_FAST_WAVES; w++) {
		F.waves[w] = L.units[w % L.n_units];
		F.waves[w].slot = (uint8_t)(w / L.n_units);
	}
	F.late_from = 0xFFFFFFFFu;
	const size_t lds = L10_LDS_BYTES;
	static LwPerDeviceOnce once; // the kernels' 109 KB of dynamic LDS, opted in once per device
	const hipError_t attr_err = once.run([] {
		// (per variant in the launchers' format order: the order in which the kernels are emitted into the code object)
		const void *fns[] = {(const void *)k_long10<LW_OUT_I16_PLANAR, false, true>, (const void *)k_long10<LW_OUT_I16_INTERLEAVED, false, true>,
			(const void *)k_long10<LW_OUT_F32_INTERLEAVED, false, true>, (const void *)k_long10<LW_OUT_F32_PLANAR, false, true>,
			(const void *)k_long10<LW_OUT_I16_PLANAR, false>, (const void *)k_long10<LW_OUT_I16_INTERLEAVED, false>,
			(const void *)k_long10<LW_OUT_F32_INTERLEAVED, false>, (const void *)k_long10<LW_OUT_F32_PLANAR, false>,
			(const void *)k_mix10<LW_OUT_I16_PLANAR, 8>, (const void *)k_mix10<LW_OUT_I16_INTERLEAVED, 8>,
			(const void *)k_mix10<LW_OUT_F32_INTERLEAVED, 8>, (const void *)k_mix10<LW_OUT_F32_PLANAR, 8>,
			(const void *)k_mix10<LW_OUT_I16_PLANAR, 16>, (const void *)k_mix10<LW_OUT_I16_INTERLEAVED, 16>,
			(const void *)k_mix10<LW_OUT_F32_INTERLEAVED, 16>, (const void *)k_mix10<LW_OUT_F32_PLANAR, 16>,
			(const void *)k_long10<LW_OUT_I16_PLANAR, true>};
		for (const void *f : fns) {
			const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
			if (e != hipSuccess)
				return e;
		}
		return hipSuccess;
	});
	if (attr_err != hipSuccess)
		return attr_err;
	if (L.n_halo_items) {
		F.items = L.d_halo_items;
		F.n_items = L.n_halo_items;
		F.per_round = 1; // spread the few halo packets over the whole chip: one packet per workgroup
		F.rounds = 1;
		const hipError_t e = lw_launch_k(k_long10<LW_OUT_I16_PLANAR, true>, dim3(L.n_halo_items), dim3(LW_WG), lds, st, F);
		if (e != hipSuccess)
			return e;
	}
	if (!L.n_items)
		return hipSuccess;
	F.items = L.d_items;
	F.n_items = L.n_items;
	F.per_round = L.per_round;
	F.rounds = L.rounds;
	F.dense = L.dense;
	F.late_from = L10_PACE;
	const uint32_t chunk = L.per_round * L.rounds;
	grid = dim3((L.n_items + chunk - 1) / chunk);
	return hipSuccess;
}
