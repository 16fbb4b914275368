// k_long12: k_long's design -- a workgroup of 16 independent waves per CU, paced HBM loads, the transform in registers, right halves
// handed from wave to wave through LDS counters, no barrier after the table image is staged -- for blocksize_1 = 12 (n = 4096).
// Included at the end of lw_kernels_long.hip (it uses that file's packed-arithmetic blocks, register transposes and stores).
//
// One wave = one CHANNEL of one packet, 1024 complex pairs = 16 per lane (lw_fast.hpp: LwL12Layout; tests/long12_model.py is the
// executable specification, bit-exact against the oracle on the CPU).  Step 1 runs on the coalesced load layout (lane holds float4
// 64 x + lane, x = 0 .. 7; the pairs 1023 - m come from the mirror lane), step 2 (pair bit 9) is register-local, and from there the
// channel is two independent 512-pair problems H0 / H1 that go through k_long's layouts B -> C -> D with k_long's register <-> lane
// exchanges (t2_inreg, t3_inreg) -- three stages in B (l = 0 .. 2), three in C (l = 3 .. 5), the fused last three in D.  They meet
// again in the bit-reverse gather through the wave's 8 KB of LDS (conflict-free slots), after which a lane finishes the four
// m' = 128 h + 2 lane + c2: steps 7 and 8, window / overlap-add, conversion, 16-byte coalesced stores.
// The two channels of a coupling step are two waves (LW_UNIT_SPLIT_*): both load both residue vectors and decouple (audio.rs:762-777),
// each keeps its own channel.  The stage tables that every lane reads per (stage, register) -- step 2, the stage twiddles, C, B, the
// window -- are staged in LDS (30 KB); the step-1 twiddles (the A table itself, 16 float2 per lane) and the floor's static interval
// indices come from HBM / L2 with the wave's other loads.
// LDS per wave: 8 KB -- first the floor's interval table (upper half), then the gather, then (lower half) the right half published
// for the successor wave: the next round's gather waits until that has been read (ACK counter).
typedef LwL12Layout Y12;
#define L12_G_BYTES 8192u
#define L12_LDS_BYTES (Y12::TOTAL + LW_FAST_WAVES * L12_G_BYTES + 3 * LW_FAST_WAVES * 4)
#define L12_CNT_BASE (Y12::TOTAL + LW_FAST_WAVES * L12_G_BYTES)
#define L12_CNT_PUB(w) (L12_CNT_BASE + 4u * (w))
#define L12_CNT_ACK(w) (L12_CNT_BASE + 4u * (LW_FAST_WAVES + (w)))
#define L12_CNT_LANDED(w) (L12_CNT_BASE + 4u * (2 * LW_FAST_WAVES + (w)))
#ifndef L12_PACE
#define L12_PACE 1             // wave w requests its residues when wave w - L12_PACE has requested its own
#endif
#ifndef L12_IMDCT_PRIO_LATE
#define L12_IMDCT_PRIO_LATE 12
#endif
static_assert(Y12::TOTAL % 16u == 0 && Y12::TOTAL / 16u <= 3u * (LW_WG - 256), "image staging below: three rows of 16 bytes per thread of 12 waves");
static_assert(L12_LDS_BYTES <= 160u * 1024u, "the image and the waves' areas fit a CU's LDS");

struct Pref12 {          // what one wave loads from HBM for one item
	float4_t r[8];       // residues of its channel: lane holds float4 64 x + lane
	float4_t pr[8];      // its partner's (coupled channels only)
	uint2_t sid[8];      // 16 * (static interval index) of its 32 bins, 4 u16 per x
	uint32_t fe;         // floor-1 post entry of post `lane` (lanes >= F hold 0)
};

template <bool COUPLED>
__device__ __forceinline__ void issue_loads12(const LwFastArgs &F, const ItemRegs &it, const LwFastUnit &un, uint32_t lane, Pref12 &p)
{
	const uint16_t *f0 = F.floors + it.floor_off + (uint32_t)un.ch_a * F.fstride;
	p.fe = lane < un.F_a ? (uint32_t)f0[lane] : 0u;
	const float4_t *s0 = reinterpret_cast<const float4_t *>(F.residue + it.res_off + (uint32_t)un.ch_a * 2048u);
	if (COUPLED) { // (both waves of the pair read both vectors: ordinary loads, the second reader finds them in L2)
		const float4_t *s1 = reinterpret_cast<const float4_t *>(F.residue + it.res_off + (uint32_t)un.ch_b * 2048u);
#pragma unroll
		for (int x = 0; x < 8; x++)
			p.r[x] = s0[64 * x + lane];
#pragma unroll
		for (int x = 0; x < 8; x++)
			p.pr[x] = s1[64 * x + lane];
	} else {
#pragma unroll
		for (int x = 0; x < 8; x++) {
			p.r[x] = __builtin_nontemporal_load(&s0[64 * x + lane]);
			asm volatile("" : "=v"(p.pr[x])); // (never read: defined, so that no earlier value is kept alive for it)
		}
	}
	const uint2_t *sd = reinterpret_cast<const uint2_t *>(F.sid12) + ((uint32_t)un.floor_a * 8u) * 64u + lane;
#pragma unroll
	for (int x = 0; x < 8; x++)
		p.sid[x] = sd[64 * x];
}

__device__ __forceinline__ void dense_offsets12(const LwFastArgs &F, uint32_t item, ItemRegs &it)
{
	it.res_off = item * F.ch * 2048u;
	it.floor_off = item * F.ch * F.fstride;
}

// interval table of the channel, lanes = posts (see floor_table: the same entry {dy, c0, 1/adx, w})
__device__ __forceinline__ bool floor_table12(const char *img, char *tab, uint32_t lane, uint32_t e, uint32_t fslot, uint32_t Fp)
{
	const bool unused = __builtin_amdgcn_readfirstlane(e) == LW_FLOOR_UNUSED;
	const unsigned long long M = __ballot((e & LW_POST_ACTIVE) != 0);
	const unsigned long long lowmask = (2ull << lane) - 1ull;
	const unsigned long long below = M & lowmask, above = M & ~lowmask;
	const int lo = below ? 63 - __builtin_clzll(below) : 0;
	const int hi = above ? __builtin_ctzll(above) : lo;
	const int y = (int)(e & 0xffu);
	const float xs = *reinterpret_cast<const float *>(img + Y12::XSF + 4u * (64u * fslot + lane));
	const int ylo = __builtin_amdgcn_ds_bpermute(lo << 2, y);
	const int yhi = __builtin_amdgcn_ds_bpermute(hi << 2, y);
	const float xlo = __int_as_float(__builtin_amdgcn_ds_bpermute(lo << 2, __float_as_int(xs)));
	const float xhi = __int_as_float(__builtin_amdgcn_ds_bpermute(hi << 2, __float_as_int(xs)));
	const float dy = (float)(yhi - ylo); // 0 when there is no later active post (flat, audio.rs:546-548)
	const float adx = above ? xhi - xlo : 1.0f;
	const bool down = yhi < ylo;
	float4_t ent;
	ent.x = dy;
	ent.y = down ? (0.875f * adx - 0.5f) - xhi * dy : (0.5f - 0.125f * adx) - xlo * dy; // exact (tests/test_big_model.py: adx <= 4096)
	ent.z = above ? __builtin_amdgcn_rcpf(adx) : 1.0f;
	ent.w = (float)(down ? yhi : ylo) + LW_FLOOR_W0;
	if (lane < Fp)
		*reinterpret_cast<float4_t *>(tab + 16 * lane) = ent;
	return unused;
}

__device__ __forceinline__ float floor_bin12(float kf, float4_t ent)
{
	const float t = __builtin_fmaf(__builtin_fmaf(kf, ent.x, ent.y), ent.z, ent.w);
	return lds_abs_f32(Y12::INV_DB - 4u + (__float_as_uint(t) & LW_FLOOR_MASK));
}

// ---- spectrum = floor x residue in place (audio.rs:1035-1037): the 32 bins 4 (64 x + lane) + j of this wave's channel
__device__ __forceinline__ void spectrum12(const char *tab, uint32_t lane, bool unused, const uint2_t (&sid)[8], float4_t (&r)[8])
{
	if (unused) {
#pragma unroll
		for (int x = 0; x < 8; x++)
			r[x] = r[x] * 0.0f; // zero floor (audio.rs:1021-1024): 0.0 x residue keeps the residue's sign
		return;
	}
	const float kf0 = (float)(4 * (int)lane);
#pragma unroll
	for (int x = 0; x < 8; x++) {
		const uint2_t sw = sid[x];
		const uint32_t s16[4] = {sw.x & 0xffffu, sw.x >> 16, sw.y & 0xffffu, sw.y >> 16};
		float4_t fl;
#pragma unroll
		for (int j = 0; j < 4; j++)
			fl[j] = floor_bin12(kf0 + (float)(256 * x + j), lds4(tab, s16[j]));
		const float2_t lo2 = pk_mul(float2_t{fl.x, fl.y}, float2_t{r[x].x, r[x].y});
		const float2_t hi2 = pk_mul(float2_t{fl.z, fl.w}, float2_t{r[x].z, r[x].w});
		r[x] = float4_t{lo2.x, lo2.y, hi2.x, hi2.y};
		if (x & 1)
			__builtin_amdgcn_sched_barrier(0); // (two x in flight at a time: hoisting all 32 interval gathers costs 128 registers)
	}
}

// ---- the inverse coupling of a pair's two vectors on the wave that keeps `r` (see spectrum_fused<1, SPLIT>)
__device__ __forceinline__ void decouple12(uint32_t coupled, float4_t (&r)[8], float4_t (&pr)[8])
{
#pragma unroll
	for (int x = 0; x < 8; x++) {
		// decouple4 wants (magnitude, angle); this wave's channel is the magnitude (LW_UNIT_SPLIT_MAG) or the angle (.._ANG)
		const bool ang = coupled == LW_UNIT_SPLIT_ANG;
		float m[4], a[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			m[j] = ang ? pr[x][j] : r[x][j];
			a[j] = ang ? r[x][j] : pr[x][j];
		}
		decouple4(m[0], a[0], m[1], a[1], m[2], a[2], m[3], a[3]);
#pragma unroll
		for (int j = 0; j < 4; j++)
			r[x][j] = ang ? a[j] : m[j];
	}
}

// ---- one 512-pair half in layout B (H[x] = pair 64 x + lane of the half): stages l = 0 .. 5, the fused last three, layout D
struct Tw12 {
	float2_t l0[4], l1[2], l2, l3[4], l4[2], l5, a2;
};

__device__ __forceinline__ void half12(const Tw12 &t, float2_t (&H)[8])
{
	bfly2x4(H[4], H[0], t.l0[0], H[5], H[1], t.l0[1], H[6], H[2], t.l0[2], H[7], H[3], t.l0[3]); // l = 0 (pair bit 8)
	bfly2x4(H[2], H[0], t.l1[0], H[6], H[4], t.l1[0], H[3], H[1], t.l1[1], H[7], H[5], t.l1[1]); // l = 1
	bfly2x4(H[1], H[0], t.l2, H[3], H[2], t.l2, H[5], H[4], t.l2, H[7], H[6], t.l2);             // l = 2
	t2_inreg(H);                                                                                 // -> C: register = p[5:3]
	bfly2x4(H[4], H[0], t.l3[0], H[5], H[1], t.l3[1], H[6], H[2], t.l3[2], H[7], H[3], t.l3[3]); // l = 3
	bfly2x4(H[2], H[0], t.l4[0], H[6], H[4], t.l4[0], H[3], H[1], t.l4[1], H[7], H[5], t.l4[1]); // l = 4
	bfly2x4(H[1], H[0], t.l5, H[3], H[2], t.l5, H[5], H[4], t.l5, H[7], H[6], t.l5);             // l = 5
	t3_inreg(H);                                                                                 // -> D: register = p[2:0]
	stage_d_block(t.a2, H);                                                                      // imdct.rs:234-288
}

// ---- the transform of the wave's channel (imdct.rs:291-659 with n = 4096): spectrum X (load layout) -> R[k4][k] = (pa, pb) at
//      q = 1023 - 2m', 1022 - 2m', 1 + 2m', 2m' for m' = 128 (k4 >> 1) + 2 lane + (k4 & 1)
//      wait_ack: the wave's published right half of the previous round lies in the lower half of G until its reader is done
__device__ __forceinline__ void imdct12(const char *img, char *G, uint32_t lane, const float2_t *apair, const float4_t (&X)[8],
		float2_t (&R)[4][4], uint32_t ack_addr, uint32_t ack_need)
{
	float2_t Q[16];
	{
		float2_t au[8], al[8], U[8];
#pragma unroll
		for (int x = 0; x < 8; x++) {
			const uint32_t m = 64u * x + lane;
			au[x] = apair[m];          // (A[2m], A[2m+1])
			al[x] = apair[1023u - m];  // (A[2046-2m], A[2047-2m])
		}
#pragma unroll
		for (int x = 0; x < 8; x += 2)
			step1x2(X[x], au[x], al[x], X[x + 1], au[x + 1], al[x + 1], U[x], Q[x], U[x + 1], Q[x + 1]);
		const uint32_t mirror = (63u - lane) << 2;
#pragma unroll
		for (int x = 0; x < 8; x++) { // pair 1023 - m lives on the mirror lane
			Q[15 - x].x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(U[x].x)));
			Q[15 - x].y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(U[x].y)));
		}
	}
	__builtin_amdgcn_sched_barrier(0); // (the table reads of the later stages must not be hoisted into step 1: registers)
	{
		float2_t s2[8];
#pragma unroll
		for (int x = 0; x < 8; x++)
			s2[x] = lds2(img + Y12::TW_S2, 8u * (64u * x + lane));
		bfly2x4(Q[8], Q[0], s2[0], Q[9], Q[1], s2[1], Q[10], Q[2], s2[2], Q[11], Q[3], s2[3]);   // step 2 (imdct.rs:385-430)
		bfly2x4(Q[12], Q[4], s2[4], Q[13], Q[5], s2[5], Q[14], Q[6], s2[6], Q[15], Q[7], s2[7]);
	}
	__builtin_amdgcn_sched_barrier(0);
	Tw12 t;
	{
		const uint32_t lo3 = lane & 7u;
#pragma unroll
		for (int y = 0; y < 4; y++) {
			t.l0[y] = lds2(img + Y12::TW_L0, 8u * (64u * y + lane));
			t.l3[y] = lds2(img + Y12::TW_L3, 8u * (8u * y + lo3));
		}
#pragma unroll
		for (int b = 0; b < 2; b++) {
			t.l1[b] = lds2(img + Y12::TW_L1, 8u * (64u * b + lane));
			t.l4[b] = lds2(img + Y12::TW_L4, 8u * (8u * b + lo3));
		}
		t.l2 = lds2(img + Y12::TW_L2, 8u * lane);
		t.l5 = lds2(img + Y12::TW_L5, 8u * lo3);
		const float a2s = *reinterpret_cast<const float *>(img + Y12::A2);
		t.a2 = float2_t{a2s, a2s};
	}
	float2_t(&H0)[8] = *reinterpret_cast<float2_t(*)[8]>(&Q[0]);
	float2_t(&H1)[8] = *reinterpret_cast<float2_t(*)[8]>(&Q[8]);
	half12(t, H0);
	__builtin_amdgcn_sched_barrier(0);
	half12(t, H1);
	__builtin_amdgcn_sched_barrier(0);
	// ---- bit-reverse gather: pair p -> slot (p >> 3 & 31) | (p & 7) << 5 | (p >> 8) << 8; layout D: lane = p[8:3], register = p[2:0]
	lds_wait_ge(ack_addr, ack_need);
	{
		char *w = G + 8u * ((lane & 31u) + 256u * (lane >> 5));
#pragma unroll
		for (int zz = 0; zz < 8; zz++) {
			*reinterpret_cast<float2_t *>(w + 256 * zz) = H0[zz];
			*reinterpret_cast<float2_t *>(w + 4096 + 256 * zz) = H1[zz];
		}
	}
	lds_fence();
	// pair 2v, v = rev8(m'): slot rev5(lane & 31) | (lane >> 5) << 7 | h << 6 | c2 << 8; 2v + 512: + 512; 511 - 2v, 1023 - 2v: 511 / 1023 minus it
	const uint32_t sa = 8u * ((__builtin_bitreverse32(lane & 31u) >> 27) + 128u * (lane >> 5));
#pragma unroll
	for (int k4 = 0; k4 < 4; k4++) { // bit-reverse gather (imdct.rs:490-528), step 7 (:533-580), step 8 (:589-658)
		const uint32_t off = 8u * (64u * (k4 >> 1) + 256u * (k4 & 1));
		const float2_t pq = lds2(G, sa + off), pqh = lds2(G, sa + off + 4096u);
		const float2_t ph = lds2(G, 4088u - off - sa), pf = lds2(G, 8184u - off - sa);
		const float4_t Cq = lds4(img + Y12::C4, 16u * (64u * k4 + lane));
		const float4_t Bl = lds4(img + Y12::B_LO, 16u * (64u * k4 + lane)), Bh = lds4(img + Y12::B_HI, 16u * (64u * k4 + lane));
		step78_block(pf, pq, ph, pqh, Cq, Bl, Bh, R[k4]);
		if (k4 & 1)
			__builtin_amdgcn_sched_barrier(0);
	}
	lds_fence();
}

// raw halves at this lane's q positions of output half h: lo = q in [256 h + 4 lane, +4), hi = q in [1020 - 256 h - 4 lane, +4)
#define L12_LO(R_, h, f) float4_t{R_[2 * (h)][3].f, R_[2 * (h)][2].f, R_[2 * (h) + 1][3].f, R_[2 * (h) + 1][2].f}
#define L12_HI(R_, h, f) float4_t{R_[2 * (h) + 1][1].f, R_[2 * (h) + 1][0].f, R_[2 * (h)][1].f, R_[2 * (h)][0].f}

// previous right half as the overlap-add consumes it: pp[k4][0] = (k = 0, k = 1), pp[k4][1] = (k = 2, k = 3)
struct PrevHalf12 {
	float2_t pp[4][2];
};

__device__ __forceinline__ void prev_from_global12(const float *g, uint32_t lane, PrevHalf12 &p)
{
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const float4_t g0 = *reinterpret_cast<const float4_t *>(g + 256u * h + 4u * lane);
		const float4_t g1 = *reinterpret_cast<const float4_t *>(g + 1020u - 256u * h - 4u * lane);
		p.pp[2 * h][1] = float2_t{g0.y, g0.x};
		p.pp[2 * h + 1][1] = float2_t{g0.w, g0.z};
		p.pp[2 * h + 1][0] = float2_t{g1.y, g1.x};
		p.pp[2 * h][0] = float2_t{g1.w, g1.z};
	}
}

// ---- window + overlap-add (audio.rs:1116-1118), sample conversion (samples.rs:92-103), stores of the wave's channel
//      (mch: samples per channel of the packet -- 2048, or 3072 - E for a block with a short right slope, EDGE)
template <int FMT>
__device__ __forceinline__ void ola_store12(const LwFastArgs &F, const char *img, uint32_t lane, uint32_t chn, uint32_t out_off, uint32_t mch,
		const float2_t (&R)[4][4], const PrevHalf12 &ph)
{
#pragma unroll
	for (int h = 0; h < 2; h++) {
		float2_t O[2][4];
#pragma unroll
		for (int c2 = 0; c2 < 2; c2++) {
			const float4_t w0 = lds4(img + Y12::WIN, 32u * (64u * (2 * h + c2) + lane));
			const float4_t w1 = lds4(img + Y12::WIN, 32u * (64u * (2 * h + c2) + lane) + 16u);
			ola_block<!lw_out_f32(FMT)>(R[2 * h + c2], ph.pp[2 * h + c2][0], ph.pp[2 * h + c2][1], w0, w1, O[c2]);
		}
		const uint32_t pos[4] = {256u * h + 4u * lane, 1020u - 256u * h - 4u * lane, 1024u + 256u * h + 4u * lane, 2044u - 256u * h - 4u * lane};
		const LwQuads q = pcm_quads(O);
#pragma unroll
		for (int g = 0; g < 4; g++)
			pcm_store4<FMT>(F.out, out_off, lw_out_itl(FMT) ? chn : chn * mch, pos[g], F.ch, q.v[g]);
	}
}

// ---- raw right half of the channel to a [2048]-float block (state slot / td block): q ascending, then mirrored
__device__ __forceinline__ void store_right_half12(float *dst, uint32_t lane, const float2_t (&R)[4][4])
{
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const float4_t lo = L12_LO(R, h, y), hi = L12_HI(R, h, y);
		store16_wt(dst + 256u * h + 4u * lane, lo);
		store16_wt(dst + 1020u - 256u * h - 4u * lane, hi);
		store16_wt(dst + 1024u + 256u * h + 4u * lane, float4_t{hi.w, hi.z, hi.y, hi.x});
		store16_wt(dst + 2044u - 256u * h - 4u * lane, float4_t{lo.w, lo.z, lo.y, lo.x});
	}
}

// EDGE (the stream's short blocks of 256 / 512 points run through k_short<8 / 16>, lw_fast.hpp): a long block with a short slope on
// either side keeps floor, inverse coupling, transform and every sample outside the short overlap here and leaves the raw edge --
// E = blocksize_0 / 4 values per channel -- in the edge buffer for k_short, exactly as k_long<EDGE> / k_long10<EDGE> do.
template <int FMT, bool RIGHT_ONLY, bool EDGE = false>
__global__ void __launch_bounds__(LW_WG) k_long12(LwFastArgs F)
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
	asm volatile("" ::"s"(F.residue), "s"(F.floors), "s"(F.n_items), "s"(n_units), "s"(per_round), "s"(rounds), "s"(F.dense),
			"s"(F.late_from), "s"(F.ch), "s"(F.fstride), "s"(F.image), "s"(unit_word));
	__builtin_memcpy(&un, &unit_word, 8);
	const uint32_t slot = un.slot, uidx = wave - slot * n_units; // packet slot of the round, unit (= channel) of the packet
	const bool active = slot < per_round;
	const uint32_t item0 = blockIdx.x * per_round * rounds + slot; // item of round j = item0 + j * per_round
	const bool coupled = un.coupled >= LW_UNIT_SPLIT_MAG;           // ch_b = the partner whose residues are loaded for the inverse coupling
	const uint32_t chn = (uint32_t)un.ch_a;
	const bool late = !RIGHT_ONLY && wave >= (F.late_from > LW_PRE_WAVES ? F.late_from : (uint32_t)LW_PRE_WAVES);

	// ---- round 0: table image (L2-resident) and residues / floors (HBM); early waves queue their HBM loads first
	ItemRegs it{};
	Pref12 pf{};
	bool valid = active && item0 < F.n_items;
	if (valid) {
		if (F.dense)
			dense_offsets12(F, item0, it);
		else
			it = load_item(F.items, item0);
	}
#define L12_ISSUE(IT)                                            \
	do {                                                         \
		if (coupled)                                             \
			issue_loads12<true>(F, IT, un, lane_id, pf);         \
		else                                                     \
			issue_loads12<false>(F, IT, un, lane_id, pf);        \
	} while (0)
	if (wave < 4) {
		if (valid && !late)
			L12_ISSUE(it);
	} else {
		const uint32_t t = threadIdx.x - 256u;
		const uint4 *src = reinterpret_cast<const uint4 *>(F.image) + t;
		uint4 *dst = reinterpret_cast<uint4 *>(smem) + t;
		constexpr uint32_t ROWS = Y12::TOTAL / 16u, STEP = LW_WG - 256;
		const uint4 v0 = src[0], v1 = src[STEP];
		uint4 v2 = make_uint4(0, 0, 0, 0);
		if (t + 2 * STEP < ROWS)
			v2 = src[2 * STEP];
		if (t < 3 * LW_FAST_WAVES)
			lds_store_u32(L12_CNT_BASE + 4u * t, 0u);
		dst[0] = v0;
		dst[STEP] = v1;
		if (t + 2 * STEP < ROWS)
			dst[2 * STEP] = v2;
		lds_fence();
		if (valid && !late)
			L12_ISSUE(it);
	}
	__syncthreads();
	const char *img = smem;
	char *G0 = smem + Y12::TOTAL; // [wave][L12_G_BYTES]
	char *G = G0 + wave * L12_G_BYTES;
	const float2_t *apair = reinterpret_cast<const float2_t *>(F.tabA);
	const bool paced = !RIGHT_ONLY && F.late_from < LW_FAST_WAVES;
	if (paced) {
		__builtin_amdgcn_s_setprio(LW_PRIO_PACE);
		if (late) {
			lds_wait_ge(L12_CNT_LANDED(wave - F.late_from), 1u);
			if (valid)
				L12_ISSUE(it);
		}
		if (wave + F.late_from < LW_FAST_WAVES) {
			asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW_PACE_VMCNT) : "memory");
			lds_store_u32(L12_CNT_LANDED(wave), 1u);
		}
		__builtin_amdgcn_s_setprio(0);
	}
	if (valid && F.dense)
		it = load_item(F.items, item0);
	uint32_t n_pub_used = 0; // hand-overs published by this wave (only those a successor reads are published)
	uint32_t n_got = 0;      // hand-overs consumed from the predecessor wave
	const uint32_t wprev = slot != 0 ? wave - n_units : (per_round - 1) * n_units + uidx;

	for (uint32_t j = 0; j < rounds; j++) {
		uint32_t lane = lane_id;
		asm volatile("" : "+v"(lane)); // (laundered once per round: see lw_long_body.inc)
		float2_t R[4][4]; // [k4][k] = (pa, pb) at q_k(m'): un-windowed left / right halves of the wave's channel
		const uint32_t item_n = item0 + (j + 1) * per_round;
		const bool valid_n = active && j + 1 < rounds && item_n < F.n_items;
		ItemRegs itn{};
		if (valid_n && !F.dense)
			itn = load_item(F.items, item_n);
		if (valid) {
			// ---- spectrum: interval table (upper half of G), inverse coupling, floor x residue
			__builtin_amdgcn_s_setprio(LW_PRIO_FLOOR);
			const bool unused = floor_table12(img, G + 4096, lane, pf.fe, un.floor_a, un.F_a);
			lds_fence();
			if (coupled)
				decouple12(un.coupled, pf.r, pf.pr);
			spectrum12(G + 4096, lane, unused, pf.sid, pf.r);
			lds_fence();
			if (wave >= L12_IMDCT_PRIO_LATE)
				__builtin_amdgcn_s_setprio(LW_PRIO_IMDCT + 1);
			else
				__builtin_amdgcn_s_setprio(LW_PRIO_IMDCT);
			imdct12(img, G, lane, apair, pf.r, R, L12_CNT_ACK(wave), n_pub_used);
			if (RIGHT_ONLY) {
				float *dst = F.halo + ((size_t)it.halo_out * F.ch + chn) * 1024u;
#pragma unroll
				for (int h = 0; h < 2; h++) {
					*reinterpret_cast<float4_t *>(dst + 256u * h + 4u * lane) = L12_LO(R, h, y);
					*reinterpret_cast<float4_t *>(dst + 1020u - 256u * h - 4u * lane) = L12_HI(R, h, y);
				}
			} else {
				__builtin_amdgcn_s_setprio(LW_PRIO_FINISH); // finish: hand-over, overlap-add, stores
				// ---- the previous packet's right half: from my predecessor wave through LDS, or (chunk starts) from the stream's
				//      state slot / the halo buffer / a generic predecessor's time-domain block -- read BEFORE this wave publishes
				//      (its own published half lies where the gather was; the predecessor's lies in the predecessor's area)
				PrevHalf12 ph;
				if (it.src_kind == LW_SRC_LDS) {
					++n_got;
					lds_wait_ge(L12_CNT_PUB(wprev), n_got);
					const char *src = G0 + wprev * L12_G_BYTES;
#pragma unroll
					for (int k4 = 0; k4 < 4; k4++) {
						const float4_t v = *reinterpret_cast<const float4_t *>(src + 16u * (64u * k4 + lane));
						ph.pp[k4][0] = float2_t{v.x, v.y};
						ph.pp[k4][1] = float2_t{v.z, v.w};
					}
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					lds_store_u32(L12_CNT_ACK(wprev), n_got);
				} else if (it.src_kind != LW_SRC_NONE) {
					const float *g;
					uint32_t cstride;
					if (it.src_kind == LW_SRC_STATE) {
						const uint32_t pin = (it.flags & LW_RF_PARITY_IN) ? 1u : 0u;
						g = F.state + ((size_t)it.src_arg * 2 + pin) * F.state_stride;
						cstride = F.state_chan_stride;
					} else if (it.src_kind == LW_SRC_HALO) {
						g = F.halo + (size_t)it.src_arg * F.ch * 1024u;
						cstride = 1024u;
					} else { // LW_SRC_TD: second half of the predecessor's [ch][4096] time-domain block
						g = F.td + (size_t)it.src_arg + 2048u;
						cstride = 4096u;
					}
					prev_from_global12(g + chn * cstride, lane, ph);
				}
				// ---- publish my right half (lower half of G: the gather has been read): the successor wave waits for the counter
				if (it.flags & LW_IF_NEXT_LDS) {
#pragma unroll
					for (int k4 = 0; k4 < 4; k4++)
						*reinterpret_cast<float4_t *>(G + 16u * (64u * k4 + lane)) = float4_t{R[k4][0].y, R[k4][1].y, R[k4][2].y, R[k4][3].y};
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					n_pub_used++;
					lds_store_u32(L12_CNT_PUB(wave), n_pub_used);
				}
				// EDGE: geometry of a long block with a short slope on the left (the window starts at 1024 - E, the first 2 E samples
				// are k_short's) and / or on the right (samples up to 3072 - E, a right part of 2 E values); E = blocksize_0 / 4
				const bool edge_l = EDGE && (it.flags & LW_IF_EDGE_L), edge_r = EDGE && (it.flags & LW_IF_EDGE_R);
				const uint32_t E = EDGE ? F.edge_n : 0u;
				const uint32_t e_ls = edge_l ? 1024u - E : 0u, e_m = EDGE ? (edge_r ? 3072u - E : 2048u) - e_ls : 2048u;
				if (it.src_kind != LW_SRC_NONE)
					ola_store12<FMT>(F, img, lane, chn, it.out_off, e_m, R, ph);
				if (EDGE && (edge_l || edge_r)) {
					// ---- short slopes: the un-windowed samples past them, the raw edges for k_short, the short state
					const bool inner = lane >= E / 4u; // this lane's q in [1020 - 4 lane, +4) lies below 1024 - E
					const bool sound = !(it.flags & LW_IF_SILENT); // (the first packet of a stream yields no samples at all)
					float *edge = F.edge + ((size_t)it.pkt * 2u * F.ch + chn) * E;
					if (edge_l) {
						// cur[2047 - q] = -pa(q) for q < 1024 - E (imdct.rs:589-658): positions 1024 + E .. 2047
#pragma unroll
						for (int h = 0; h < 2; h++) {
							const float4_t lo = L12_LO(R, h, x), hi = L12_HI(R, h, x);
							store_quad<FMT>(F, (int)chn, it.out_off, e_m, 2044u - 256u * h - 4u * lane - e_ls, float4_t{-lo.w, -lo.z, -lo.y, -lo.x}, sound);
							store_quad<FMT>(F, (int)chn, it.out_off, e_m, 1024u + 256u * h + 4u * lane - e_ls, float4_t{-hi.w, -hi.z, -hi.y, -hi.x},
									sound && (h == 1 || inner));
						}
						if (!inner) // raw left edge pa(1024 - E + i), i = E - 4 - 4 lane ..
							store16_wt(edge + (E - 4u) - 4u * lane, L12_HI(R, 0, x));
					}
					if (edge_r) {
						// cur[2048 + q] = pb(q) for q < 1024 - E: positions 2048 .. 3071 - E
#pragma unroll
						for (int h = 0; h < 2; h++) {
							const float4_t lo = L12_LO(R, h, y), hi = L12_HI(R, h, y);
							store_quad<FMT>(F, (int)chn, it.out_off, e_m, 2048u + 256u * h + 4u * lane - e_ls, lo, sound);
							store_quad<FMT>(F, (int)chn, it.out_off, e_m, 3068u - 256u * h - 4u * lane - e_ls, hi, sound && (h == 1 || inner));
						}
						if (!inner) { // raw right part cur[3072 - E .. 3072 + E): pb(1024 - E + i), then mirrored
							const float4_t hi = L12_HI(R, 0, y);
							store16_wt(edge + (size_t)F.ch * E + (E - 4u) - 4u * lane, hi);
							if (it.state_out >= 0) {
								float *dst = F.state + ((size_t)it.state_out * 2 + ((it.flags & LW_RF_PARITY_OUT) ? 1u : 0u)) * F.state_stride +
									chn * F.state_chan_stride;
								store16_wt(dst + (E - 4u) - 4u * lane, hi);
								store16_wt(dst + E + 4u * lane, float4_t{hi.w, hi.z, hi.y, hi.x});
							}
						}
					}
				}
				// ---- raw right half to the stream's state slot and / or to the td block a generic successor reads
				if (it.state_out >= 0 && !edge_r) {
					const uint32_t pout = (it.flags & LW_RF_PARITY_OUT) ? 1u : 0u;
					store_right_half12(F.state + ((size_t)it.state_out * 2 + pout) * F.state_stride + chn * F.state_chan_stride, lane, R);
				}
				if (it.flags & LW_RF_WRITE_TD)
					store_right_half12(F.td + 2u * (size_t)it.res_off + chn * 4096u + 2048u, lane, R);
				if (EDGE && (it.flags & LW_IF_TDONLY)) {
					// a block whose window / overlap-add k_ola_generic does (short slopes without an edge form): the un-windowed left
					// half too -- cur[q] = pa(q), cur[2047 - q] = -pa(q) (imdct.rs:589-658)
					float *dst = F.td + 2u * (size_t)it.res_off + chn * 4096u;
#pragma unroll
					for (int h = 0; h < 2; h++) {
						const float4_t lo = L12_LO(R, h, x), hi = L12_HI(R, h, x);
						store16_wt(dst + 256u * h + 4u * lane, lo);
						store16_wt(dst + 1020u - 256u * h - 4u * lane, hi);
						store16_wt(dst + 1024u + 256u * h + 4u * lane, float4_t{-hi.w, -hi.z, -hi.y, -hi.x});
						store16_wt(dst + 2044u - 256u * h - 4u * lane, float4_t{-lo.w, -lo.z, -lo.y, -lo.x});
					}
				}
			}
		}
		__builtin_amdgcn_s_setprio(0);
		// ---- HBM loads of the next round
		if (valid_n) {
			if (F.dense) {
				dense_offsets12(F, item_n, itn);
				L12_ISSUE(itn);
				itn = load_item(F.items, item_n);
			} else {
				L12_ISSUE(itn);
			}
		} else {
			// (the old values are dead: defining them here keeps 80 registers from being carried through the transform for the path
			// that never reads them again -- 276 bytes of scratch per lane without it)
#pragma unroll
			for (int x = 0; x < 8; x++)
				asm volatile("" : "=v"(pf.r[x]), "=v"(pf.pr[x]), "=v"(pf.sid[x]));
			asm volatile("" : "=v"(pf.fe));
		}
		it = itn;
		valid = valid_n;
	}
#undef L12_ISSUE
}

hipError_t lw_launch_long12(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, int fmt, hipStream_t st)
{
	LwFastArgs F{};
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
	F.tabA = T.bs[1].A;
	F.sid12 = L.d_sid12;
	for (uint32_t w = 0; w < LW_FAST_WAVES; w++) {
		F.waves[w] = L.units[w % L.n_units];
		F.waves[w].slot = (uint8_t)(w / L.n_units);
	}
	F.late_from = 0xFFFFFFFFu;
	const size_t lds = L12_LDS_BYTES;
	static LwPerDeviceOnce once; // the kernels' 158 KB of dynamic LDS, opted in once per device
	const hipError_t attr_err = once.run([] {
		const void *fns[] = {(const void *)k_long12<LW_OUT_I16_PLANAR, false>, (const void *)k_long12<LW_OUT_I16_INTERLEAVED, false>,
			(const void *)k_long12<LW_OUT_F32_PLANAR, false>, (const void *)k_long12<LW_OUT_I16_PLANAR, true>,
			(const void *)k_long12<LW_OUT_I16_PLANAR, false, true>, (const void *)k_long12<LW_OUT_I16_INTERLEAVED, false, true>,
			(const void *)k_long12<LW_OUT_F32_PLANAR, false, true>, (const void *)k_long12<LW_OUT_F32_INTERLEAVED, false>,
			(const void *)k_long12<LW_OUT_F32_INTERLEAVED, false, true>};
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
		const hipError_t e = lw_launch_k(k_long12<LW_OUT_I16_PLANAR, true>, dim3(L.n_halo_items), dim3(LW_WG), lds, st, F);
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
	F.late_from = L12_PACE;
	const uint32_t chunk = L.per_round * L.rounds;
	const dim3 grid((L.n_items + chunk - 1) / chunk), block(LW_WG);
	if (L.edge_mode || L.has_tdonly) // (chosen per batch: an all-(1,1) batch keeps the plain kernel)
		return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_long12<f.value, false, true>, grid, block, lds, st, F); });
	return lw_with_out_fmt(fmt, [&](auto f) { return lw_launch_k(k_long12<f.value, false>, grid, block, lds, st, F); });
}
