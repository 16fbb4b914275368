// Body of the block kernel (see lw_kernels_long.hip: k_short).  Included textually -- once as k_short, twice as the short-block role
// of k_mix -- for the reason given in lw_long_body.inc.  The work of one wave: the (task, unit) `wid`.  Names from the including
// scope: F (LwShortArgs), smem_all (the table image; staged here when STAGE), smem (the wave's own areas behind it), wid, lane
// (0..63), the compile-time switches FMT, L, ONLY, STAGE, and edge_flags, mix_err, mix_spin (k_mix only).  ONLY >= 0 (k_mix): the wave finishes channel ONLY of
// its pair, known at compile time -- 108 registers instead of 192, so that the body fits a 16-wave workgroup -- and edge_flags
// orders it behind the long blocks' waves of the SAME launch: edge_flags[(packet * 2 + side) * ch + channel] != 0 once k_long's
// wave has written that raw edge; a wave that does not see its flags within mix_spin polls sets *mix_err and stores nothing.
	typedef LwBlkLayout<L> Y;
	typedef LwBlkLds<L> D;
	constexpr int PT = D::PT;
	constexpr bool ONE = ONLY >= 0;
	const uint32_t g = lane / L, l_id = lane % L;
	const uint32_t task = wid / F.n_units, uidx = wid - task * F.n_units;
	const LwFastUnit un = F.units[uidx];
	const bool two = un.ch_b >= 0;
	const uint32_t chn[2] = {(uint32_t)un.ch_a, (uint32_t)(two ? un.ch_b : un.ch_a)};
	// Small launches split a channel pair over two waves (un.slot = the one channel this wave finishes, 0xFF = both): the
	// launch lasts as long as one wave's dependent chain, and past the inverse coupling the channels need nothing from each
	// other.  Both waves load both residue vectors (a coupled pair) and decouple; each does floor, transform and samples
	// of its own channel only.
	const uint32_t only = ONE ? (uint32_t)ONLY : un.slot;
	const bool mine[2] = {ONE ? ONLY == 0 : only != 1u, ONE ? ONLY == 1 : (two && only != 0u)};
	// ---- the table image (L2-resident), staged by the wave that uses it.  (Workgroups of 8-12 waves sharing one image were
	// measured 6-17 % slower on every shape: their waves start together and move through the memory- and compute-bound
	// phases in lock step, and a CU takes the next workgroup only when the whole previous one is done; single waves are
	// dispatched one by one and interleave.)
	if (STAGE) {
		const uint4 *src = reinterpret_cast<const uint4 *>(F.image);
		uint4 *dst = reinterpret_cast<uint4 *>(smem_all);
		static_assert(Y::TOTAL % 1024u == 0, "whole rows of 64 lanes x 16 bytes");
		constexpr uint32_t ROUNDS = Y::TOTAL / 1024u;
		uint4 v[ROUNDS]; // all loads in flight at once: one L2 round trip for the whole image
#pragma unroll
		for (uint32_t k = 0; k < ROUNDS; k++)
			v[k] = src[lane + 64u * k];
#pragma unroll
		for (uint32_t k = 0; k < ROUNDS; k++)
			dst[lane + 64u * k] = v[k];
	}
	typedef LwBlkWave<L, ONE> W;
	constexpr uint32_t OFF_SCR = W::SCR, OFF_PUB = W::PUB, OFF_REC = W::REC, OFF_TAB = W::TAB, POSTS_ = W::POSTS, CH = W::CH;
	for (uint32_t pass = 0; pass < F.passes; pass++) {
	// launder the lane index once per pass: everything derived from it (table addresses, twiddles) is recomputed where it is
	// used instead of being hoisted out of the loop and kept in ~70 registers
	uint32_t l = l_id;
	asm volatile("" : "+v"(l));
	// ---- slot descriptor (all lanes of a group read the same 48 bytes)
	const uint4 *sp = reinterpret_cast<const uint4 *>(F.slots + (((size_t)task * F.passes + pass) * D::SLOTS + g));
	const uint4 d0 = sp[0], d1 = sp[1], d2 = sp[2];
	const uint32_t res_off = d0.x, floor_off = d0.y, out_off = d0.z, prev_arg = d0.w;
	const int32_t state_out = (int32_t)d1.x;
	const uint32_t next_edge = d1.y, next_out = d1.z, next_m = d1.w;
	const uint32_t prev_stride = d2.x & 0xffffu, kind = (d2.x >> 16) & 0xffu, prev_kind = d2.x >> 24, flags = d2.y;
	const bool has_block = kind == LW_SS_BLOCK || kind == LW_SS_HALO;
	// ---- HBM loads, all at once: floor records, residues, the previous right part and the successor's left edge
	uint32_t fe[2][PT];
	float4_t r[2][4];
	Half8 prv[2], nxt[2];
#pragma unroll
	for (int c = 0; c < 2; c++) {
		const bool on = mine[c];
		const bool need_res = (c == 0 || two) && (on || un.coupled); // (the partner's vector: for the inverse coupling only)
		const uint32_t Fp = c == 0 ? un.F_a : un.F_b;
		const uint16_t *f = F.floors + floor_off + chn[c] * F.fstride;
#pragma unroll
		for (int t = 0; t < PT; t++) {
			const uint32_t i = l + L * (uint32_t)t;
			fe[c][t] = on && has_block && i < Fp ? (uint32_t)f[i] : 0u;
		}
		const float4_t *s = reinterpret_cast<const float4_t *>(F.residue + res_off + chn[c] * (16u * L));
#pragma unroll
		for (int x = 0; x < 4; x++)
			r[c][x] = need_res && has_block ? __builtin_nontemporal_load(&s[L * x + l]) : float4_t{0.0f, 0.0f, 0.0f, 0.0f};
		// the state pool is addressed in size_t like the store below (a stream's slot lies anywhere in a pool of up to 2^31 - 1
		// slots); the edge and time-domain offsets are per-batch and stay 32-bit: lw_batch_create refuses a batch whose last
		// packet's offsets do not fit (lw_batch_max_packets)
		const float *pbase = F.state;
		size_t poff = 0;
		if (prev_kind == LW_SP_STATE) {
			poff = ((size_t)prev_arg * 2u + ((flags & LW_RF_PARITY_IN) ? 1u : 0u)) * F.state_stride + chn[c] * F.state_chan_stride;
		} else if (prev_kind == LW_SP_EDGE) {
			pbase = F.edge;
			poff = ((prev_arg * 2u + 1u) * F.ch + chn[c]) * (8u * L);
		} else if (prev_kind == LW_SP_TD) {
			pbase = F.td;
			poff = prev_arg + chn[c] * prev_stride;
		}
		prv[c].lo = prv[c].hi = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
		if (on && prev_kind >= LW_SP_STATE && !(ONE && prev_kind == LW_SP_EDGE)) // (k_mix: the raw edges are written in this launch: below)
			prv[c] = load_half8<L>(pbase + poff, l);
		nxt[c].lo = nxt[c].hi = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
		if (L <= 16 && on && next_edge != 0xFFFFFFFFu && !ONE)
			nxt[c] = load_half8<L>(F.edge + ((size_t)next_edge * 2u * F.ch + chn[c]) * (8u * L), l);
	}
	const char *img = smem_all;
	char *scr = smem + OFF_SCR, *pub = smem + OFF_PUB + (ONE ? 0u : W::PUB_PASS * (pass & 1u));
	// (the previous slot of group 0 is the last slot of the pass before: the other half of the double buffer; ONE: a single pass)
	const char *pub_prev = g != 0 ? pub + 16u * ((g - 1u) * CH * 2u * L)
		: smem + OFF_PUB + (ONE ? 0u : W::PUB_PASS * ((pass & 1u) ^ 1u)) + 16u * ((D::SLOTS - 1u) * CH * 2u * L);
	lds_fence();
	// ---- floor curves (interval entries by lanes = posts), inverse coupling, floor x residue
	bool unused[2] = {true, true};
#pragma unroll
	for (int c = 0; c < 2; c++) {
		if (!mine[c])
			continue;
		char *rec = smem + OFF_REC + (g * CH + (ONE ? 0u : c)) * (POSTS_ * 2u);
		char *tab = smem + OFF_TAB + (g * CH + (ONE ? 0u : c)) * (POSTS_ * 16u);
		unused[c] = short_floor_table<L>(img, rec, tab, g, l, fe[c], c == 0 ? un.floor_a : un.floor_b, c == 0 ? un.F_a : un.F_b, has_block);
	}
	lds_fence();
	if (two && un.coupled) {
#pragma unroll
		for (int x = 0; x < 4; x++) {
			float m[4] = {r[0][x].x, r[0][x].y, r[0][x].z, r[0][x].w};
			float a[4] = {r[1][x].x, r[1][x].y, r[1][x].z, r[1][x].w};
			decouple4(m[0], a[0], m[1], a[1], m[2], a[2], m[3], a[3]);
			r[0][x] = float4_t{m[0], m[1], m[2], m[3]};
			r[1][x] = float4_t{a[0], a[1], a[2], a[3]};
		}
	}
	float2_t R[2][2][4]; // [channel][c2][k] = (pa, pb)
#pragma unroll
	for (int c = 0; c < 2; c++) {
		if (!mine[c])
			continue;
		const char *tab = smem + OFF_TAB + (g * CH + (ONE ? 0u : c)) * (POSTS_ * 16u);
		short_spectrum<L>(img, tab, l, c == 0 ? un.floor_a : un.floor_b, unused[c], r[c]);
		short_imdct<L>(img, scr, g, l, r[c], R[c]);
		if (ONE) {
			// k_mix: the raw edges this slot needs come from long blocks' waves of the SAME launch (other workgroups): wait for
			// their flags -- everything above ran without them --, read the edges with loads that see write-through data, and
			// clear the flags for the next launch (every edge has exactly one reader)
			const bool need_prev = L <= 16 && prev_kind == LW_SP_EDGE, need_next = L <= 16 && next_edge != 0xFFFFFFFFu;
			uint32_t *fp = edge_flags + (prev_arg * 2u + 1u) * F.ch + chn[c], *fn = edge_flags + (next_edge * 2u) * F.ch + chn[c];
			bool seen = false;
			for (uint32_t spin = 0; spin < mix_spin; spin++) { // (bounded: a missing producer must not end in a hung GPU ...)
				const bool ok = (!need_prev || load_flag_coherent(fp) != 0u) && (!need_next || load_flag_coherent(fn) != 0u);
				if (__all(ok)) {
					seen = true;
					break;
				}
				__builtin_amdgcn_s_sleep(2);
			}
			if (!seen) {
				// ... and not in wrong samples either (audio.rs:27-41: every failure is a status): the wave raises the batch's
				// device error word and stores nothing; the host turns it into LW_ERR_DEVICE for the whole batch and zeroes
				// the flags (lw_batch_device_status)
				if (lane == 0)
					raise_device_error(mix_err);
				return;
			}
			if (need_prev)
				prv[c] = load_half8_coherent(F.edge + ((prev_arg * 2u + 1u) * F.ch + chn[c]) * (8u * L), l, 8u * L);
			if (need_next)
				nxt[c] = load_half8_coherent(F.edge + ((size_t)next_edge * 2u * F.ch + chn[c]) * (8u * L), l, 8u * L);
			if (l == 0) {
				if (need_prev)
					__hip_atomic_store(fp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (need_next)
					__hip_atomic_store(fn, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
		if (L <= 16 && kind == LW_SS_EDGE) { // no block of its own: the stored right part stands in for it (feeds the successor's left edge)
			R[c][0][3].y = prv[c].lo.x, R[c][0][2].y = prv[c].lo.y, R[c][1][3].y = prv[c].lo.z, R[c][1][2].y = prv[c].lo.w;
			R[c][1][1].y = prv[c].hi.x, R[c][1][0].y = prv[c].hi.y, R[c][0][1].y = prv[c].hi.z, R[c][0][0].y = prv[c].hi.w;
		}
		// right part for the next slot of the wave: [slot][channel][c2][l] float4 = pb at k = 0..3
#pragma unroll
		for (int c2 = 0; c2 < 2; c2++)
			*reinterpret_cast<float4_t *>(pub + 16u * (((g * CH + (ONE ? 0u : c)) * 2u + c2) * L + l)) =
				float4_t{R[c][c2][0].y, R[c][c2][1].y, R[c][c2][2].y, R[c][c2][3].y};
	}
	lds_fence();
	// ---- window / overlap-add / stores of the slot's own samples; state; the successor's left edge
	const uint32_t esz_stride = lw_out_itl(FMT) ? F.ch : 1u;
#pragma unroll
	for (int c = 0; c < 2; c++) {
		if (!mine[c])
			continue;
		if (kind == LW_SS_BLOCK && prev_kind != LW_SP_NONE) {
			PrevHalf ph;
			if (prev_kind == LW_SP_LANE) {
#pragma unroll
				for (int c2 = 0; c2 < 2; c2++) {
					const float4_t v = *reinterpret_cast<const float4_t *>(pub_prev + 16u * (((ONE ? 0u : c) * 2u + c2) * L + l));
					ph.pp[c2][0] = float2_t{v.x, v.y};
					ph.pp[c2][1] = float2_t{v.z, v.w};
				}
			} else {
				prev_from_half8(prv[c], ph);
			}
			const uint32_t e0 = lw_out_itl(FMT) ? out_off + chn[c] : out_off + chn[c] * (16u * L);
			short_ola_store<FMT, L>(img, l, F.out, e0, esz_stride, R[c], ph);
		}
		if (kind == LW_SS_BLOCK && state_out >= 0)
			short_store_right<L>(F.state + ((size_t)state_out * 2u + ((flags & LW_RF_PARITY_OUT) ? 1u : 0u)) * F.state_stride +
					chn[c] * F.state_chan_stride, l, R[c]);
		if (kind == LW_SS_BLOCK && (flags & LW_SF_WRITE_TD))
			short_store_right<L>(F.td + 2u * (size_t)res_off + chn[c] * (32u * L) + 16u * L, l, R[c]);
		if (L <= 16 && next_edge != 0xFFFFFFFFu && (kind == LW_SS_BLOCK || kind == LW_SS_EDGE)) {
			// the long successor's first 16 L samples: its raw left edge (the top 8 L values of its pa) against this slot's right part,
			// short slope
			float2_t Rn[2][4];
			Rn[0][3].x = nxt[c].lo.x, Rn[0][2].x = nxt[c].lo.y, Rn[1][3].x = nxt[c].lo.z, Rn[1][2].x = nxt[c].lo.w;
			Rn[1][1].x = nxt[c].hi.x, Rn[1][0].x = nxt[c].hi.y, Rn[0][1].x = nxt[c].hi.z, Rn[0][0].x = nxt[c].hi.w;
			PrevHalf ph;
#pragma unroll
			for (int c2 = 0; c2 < 2; c2++) {
#pragma unroll
				for (int k = 0; k < 4; k++)
					Rn[c2][k].y = 0.0f;
				ph.pp[c2][0] = float2_t{R[c][c2][0].y, R[c][c2][1].y};
				ph.pp[c2][1] = float2_t{R[c][c2][2].y, R[c][c2][3].y};
			}
			const uint32_t e0 = lw_out_itl(FMT) ? next_out + chn[c] : next_out + chn[c] * next_m;
			short_ola_store<FMT, L>(img, l, F.out, e0, esz_stride, Rn, ph);
		}
	}
	lds_fence(); // (the next pass re-uses the record / table / gather areas)
	} // pass
