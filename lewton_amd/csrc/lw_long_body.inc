// Body of the long-block kernel (see lw_kernels_long.hip: k_long).  Included textually -- once as k_long, once as the long-block
// role of k_mix -- so that k_long's code generation does not depend on how the other kernel is built (as a function taking the
// arguments by reference the headline kernel compiled differently).  Names from the including scope: F (LwFastArgs), the
// compile-time switches FMT, RIGHT_ONLY, TD, EDGE, SPLIT, PRE, MIXF, and edge_flags, mix_drop_flags (MIXF: a wave that has written a raw
// edge sets edge_flags[(packet * 2 + side) * ch + channel] behind it, which is what the short block's wave of the same launch
// waits for).
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const uint32_t lane_id = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	LW_STAMP_DECL;
	LW_STAMP(0);
	const uint32_t n_units = F.n_units, per_round = F.per_round, rounds = F.rounds;
	// this wave's unit and packet slot: one 8-byte scalar load from the kernel-argument segment, requested together with ...
	LwFastUnit un;
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const unsigned long long __attribute__((address_space(4))) *ka_ptr;
	const unsigned long long unit_word = ((ka_ptr)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(LwFastArgs, waves) / 8 + wave];
#else
	const unsigned long long unit_word = 0;
#endif
	// ... every scalar the first HBM loads depend on: ONE batch of kernel-argument loads behind one wait (the compiler
	// would otherwise load them one by one, each behind its own s_waitcnt, on the critical path to the first load)
	asm volatile("" ::"s"(F.residue), "s"(F.floors), "s"(F.n_items), "s"(n_units), "s"(per_round), "s"(rounds), "s"(F.dense),
			"s"(F.late_from), "s"(F.ch), "s"(F.fstride), "s"(F.image), "s"(unit_word));
	__builtin_memcpy(&un, &unit_word, 8);
	const uint32_t slot = un.slot, uidx = wave - slot * n_units; // packet slot of the round, unit of the packet
	const bool active = slot < per_round;
	const uint32_t item0 = blockIdx.x * per_round * rounds + slot;      // item of round j = item0 + j * per_round
	const bool two = !SPLIT && un.ch_b >= 0; // (SPLIT: every unit is one channel; ch_b, if any, is the coupling partner whose residues are loaded)
	const int chn[2] = {un.ch_a, two ? un.ch_b : un.ch_a};
	// PRE: the coupling steps this wave evaluates itself before its unit's own (LwFastPlan::pre): their program and two more channels
	const uint32_t pre_prog = PRE ? __builtin_amdgcn_readfirstlane(F.pre[wave]) : 0u;
	PreRegs pq;
#define LW_PRE_WAVES 2 // waves that queue their HBM loads before the barrier (waves 0-3 can: the others stage the image);
                       // measured: 1 -> 17.33, 2 -> 17.0-17.16, 4 -> 17.73 us; releasing the next wave of the chain before
                       // (18.0) or half-way through (17.17) the own loads is slower than after them
	const bool late = !RIGHT_ONLY && wave >= (F.late_from > LW_PRE_WAVES ? F.late_from : (uint32_t)LW_PRE_WAVES);

	// ---- round 0: table image (L2-resident) and residues/floors (HBM); early waves queue their HBM loads first
	ItemRegs it{};
	Pref pf{};
	bool valid = active && item0 < F.n_items;
	if (valid) {
		if (F.dense)
			dense_offsets(F, item0, it);
		else
			it = load_item(F.items, item0);
	}
	// Waves 0-3 (the first pacing group) only queue their HBM loads; waves 4-15 stage the table image (1536 x 16 bytes =
	// 2 per thread, no tail) and clear the hand-over counters.  A wave that waits for image data therefore never has
	// residue loads in flight (s_waitcnt vmcnt counts in order), and the first group's loads are issued ~1 us after launch.
	static_assert(LWI_TOTAL / 16 == 2 * (LW_WG - 256), "image staging: 12 waves x 2 x 16 bytes per thread");
	static_assert(LW_FLOOR_FIRST_FROM >= 4, "floor-first waves request their floor records after staging the image");
	const bool floor_first = !PRE && late && two && F.late_from < LW_FAST_WAVES && wave >= LW_FLOOR_FIRST_FROM; // (PRE: two more vectors in flight -- no room for the floor values next to them)
	if (wave < 4) {
		if (valid && !late)
			{
				issue_loads<!PRE>(F, it, un, lane_id, pf);
				if (PRE)
					issue_pre_loads(F, it, pre_prog, lane_id, pq);
			}
	} else {
		const uint32_t t = threadIdx.x - 256u;
		const uint4 *src = reinterpret_cast<const uint4 *>(F.image) + t;
		uint4 *dst = reinterpret_cast<uint4 *>(smem) + t;
		const uint4 v0 = src[0], v1 = src[LW_WG - 256];
#ifdef LW_LONG_BODY_STAGE_LOAD
		LW_LONG_BODY_STAGE_LOAD // (k_mix: the short blocks' image is requested in the same round trip ...)
#endif
		if (t < 3 * LW_FAST_WAVES)
			lds_store_u32(LW_CNT_BASE + 4u * t, 0u);
		dst[0] = v0;
		dst[LW_WG - 256] = v1;
#ifdef LW_LONG_BODY_STAGE_STORE
		LW_LONG_BODY_STAGE_STORE // (... and stored in front of the same barrier)
#endif
		lds_fence();
		if (valid && !late)
			{
				issue_loads<!PRE>(F, it, un, lane_id, pf);
				if (PRE)
					issue_pre_loads(F, it, pre_prog, lane_id, pq);
			}
		// a floor-first wave (below) asks for its floor records now, 58 bytes per channel: behind the image data it just
		// waited for (loads return in order), ahead of every residue it will request
		if (valid && floor_first)
			issue_floor_loads(F, it, un, lane_id, pf);
	}
	__syncthreads();
#ifdef LW_LONG_BODY_AFTER_STAGE
	LW_LONG_BODY_AFTER_STAGE // (k_mix: the workgroup's last waves leave for the short blocks here)
#endif
	const char *img = smem;
	LW_STAMP(2);
	char *sc = smem + LWI_TOTAL + wave * LW_SCR_BYTES;
	char *pub0 = smem + LWI_TOTAL + LW_FAST_WAVES * LW_SCR_BYTES; // [wave][LW_PUB_BYTES]
	char *pub = pub0 + wave * LW_PUB_BYTES;
	// A wave far enough back in the load queue builds its floor curve NOW, before its turn to request residues comes (the
	// queue advances by one wave per ~0.6 us; the floor stage is ~1.8 us of LDS round trips with the VALU mostly idle):
	// when its residues land, only inverse coupling, one multiply per bin and the IMDCT are left.  The first waves of the
	// queue request their residues first (the queue must not wait for them) and build the curve afterwards.
#define LW_PACE_VMCNT 63
	// Order the HBM queue: wave w issues its loads when wave w - late_from has issued its own (LW_PACE_VMCNT = 63) or
	// has all but LW_PACE_VMCNT of them back.  Requests of one CU are served in issue order, so the data arrives
	// wave by wave instead of all at the end of the burst: the first waves compute while the later waves' data is
	// still in flight (issue order, one wave at a time, measured best: 18.7 us vs 27 us unpaced).
	const bool paced = !RIGHT_ONLY && F.late_from < LW_FAST_WAVES;
	// ---- round 0 up to the spectrum (floor x residue) in the residue registers
	// (the lane id is laundered, as in the loop below: with its known bits visible hipcc turns every `4 lane + const` of the
	// floor stage into an integer OR plus a conversion, two instructions per bin instead of one addition)
	uint32_t lane0 = lane_id;
	asm volatile("" : "+v"(lane0));
	if (valid && floor_first) {
		// (one block, so that no residue register is live during the floor stage and no floor register after it)
		float4_t fl[2][4]; // floor value of every bin this lane holds
		floor_phase<2>(F, img, sc, lane0, un, pf.fe, fl);
		LW_STAMP(1);
		__builtin_amdgcn_s_setprio(LW_PRIO_PACE);
		lds_wait_ge(LW_CNT_LANDED(wave - F.late_from), 1u);
		issue_residue_loads<true, !PRE>(F, it, un, lane0, pf);
		if (PRE)
			issue_pre_loads(F, it, pre_prog, lane0, pq);
		LW_STAMP(15);
		if (wave + F.late_from < LW_FAST_WAVES) {
			asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW_PACE_VMCNT) : "memory");
			lds_store_u32(LW_CNT_LANDED(wave), 1u);
		}
		if (F.dense)
			it = load_item(F.items, item0); // the rest of the item (phase 2); its latency hides behind the residues'
		__builtin_amdgcn_s_setprio(LW_PRIO_READY);
		LW_STAMP_W(3);
		if (PRE)
			apply_pre(pre_prog, pf, pq);
		spectrum_ready(un, pf, fl);
		__builtin_amdgcn_s_setprio(0);
		LW_STAMP(4);
	} else {
		if (paced) {
			__builtin_amdgcn_s_setprio(LW_PRIO_PACE);
			if (late) {
				lds_wait_ge(LW_CNT_LANDED(wave - F.late_from), 1u);
				if (valid)
					{
				issue_loads<!PRE>(F, it, un, lane0, pf);
				if (PRE)
					issue_pre_loads(F, it, pre_prog, lane0, pq);
			}
			}
			LW_STAMP(15);
			if (wave + F.late_from < LW_FAST_WAVES) {
				asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW_PACE_VMCNT) : "memory");
				lds_store_u32(LW_CNT_LANDED(wave), 1u);
			}
			__builtin_amdgcn_s_setprio(0);
		}
		if (valid && F.dense)
			it = load_item(F.items, item0); // the rest of the item (phase 2); its latency hides behind the residues'
		LW_STAMP_W(3);
		if (valid) {
			if (PRE)
				apply_pre(pre_prog, pf, pq);
			if (two)
				spectrum_fused<2, false, true>(F, img, sc, lane0, un, pf);
			else
				spectrum_fused<1, SPLIT>(F, img, sc, lane0, un, pf);
		}
		LW_STAMP(4);
	}
	uint32_t n_pub_used = 0; // hand-overs published by this wave (only those a successor reads are published)
	uint32_t n_got = 0;      // hand-overs consumed from the predecessor wave
	// predecessor waves: same round (slot > 0) / previous round (slot == 0)
	const uint32_t wprev = slot != 0 ? wave - n_units : (per_round - 1) * n_units + uidx;

	for (uint32_t j = 0; j < rounds; j++) {
		// launder the lane id once per round: everything derived from it (LDS addresses, bin numbers as floats) is
		// recomputed where it is used instead of being hoisted out of the loop and kept in registers
		// (in place, in the ONE register that holds the lane id from the barrier on: a laundered copy per round kept a second one occupied)
		asm volatile("" : "+v"(lane0));
		const uint32_t lane = lane0;
		float2_t R[2][2][4]; // [channel][c2][k] = (pa, pb) at q_k(m' = 2 lane + c2): un-windowed left / right halves
		const uint32_t item_n = item0 + (j + 1) * per_round;
		const bool valid_n = active && j + 1 < rounds && item_n < F.n_items;
		ItemRegs itn{};
		if (valid_n && !F.dense)
			itn = load_item(F.items, item_n);
		if (valid) {
			if (two)
				long_imdct<2, MIXF ? 1 : 0>(F, img, sc, lane, wave, pf, R);
			else
				long_imdct<1, MIXF ? 1 : 0>(F, img, sc, lane, wave, pf, R);
			if (j == 0)
				LW_STAMP(8);
		}
		if (valid) {
			if (RIGHT_ONLY) {
#pragma unroll
				for (int c = 0; c < 2; c++)
					if (c == 0 || two) {
						float *dst = F.halo + ((size_t)it.halo_out * F.ch + chn[c]) * 512u;
						char *dstb = reinterpret_cast<char *>(dst); // (wave-uniform base, 32-bit byte offsets: see store16_wt_u)
						*reinterpret_cast<float4_t *>(dstb + 16u * lane) = LW_PB_LO0(c);
						*reinterpret_cast<float4_t *>(dstb + (2032u - 16u * lane)) = LW_PB_LO1(c);
					}
			} else {
				__builtin_amdgcn_s_setprio(LW_PRIO_FINISH); // finish: hand-over, overlap-add, stores
				// EDGE kernels: geometry of a long block with a short slope on the left (window starts at 448, the first 128
				// samples are k_short's) and / or on the right (samples up to 1472, 128-sample right part)
				const bool edge_l = EDGE && (it.flags & LW_IF_EDGE_L), edge_r = EDGE && (it.flags & LW_IF_EDGE_R);
				const uint32_t e_ls = edge_l ? 448u : 0u, e_m = EDGE ? (edge_r ? 1472u : 1024u) - e_ls : 1024u;
				if (MIXF && (edge_l || edge_r)) {
					// k_mix: short blocks' waves of this very launch wait for the raw edges -- out with them first, written through,
					// and the flags behind them (the edge stores further down are skipped)
#pragma unroll
					for (int c = 0; c < 2; c++)
						if ((c == 0 || two) && lane < 16u) {
							float *edge = F.edge + ((size_t)it.pkt * 2u * F.ch + (uint32_t)chn[c]) * LW_EDGE_VALUES;
							if (edge_l)
								store16_wt(edge + 60u - 4u * lane, LW_PA_LO1(c));
							if (edge_r)
								store16_wt(edge + (size_t)F.ch * LW_EDGE_VALUES + 60u - 4u * lane, LW_PB_LO1(c));
						}
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
					if (lane == 0 && !mix_drop_flags) { // (mix_drop_flags: test hook, a producer that never signals)
#pragma unroll
						for (int c = 0; c < 2; c++)
							if (c == 0 || two) {
								uint32_t *fl = edge_flags + ((size_t)it.pkt * 2u) * F.ch + (uint32_t)chn[c];
								if (edge_l)
									__hip_atomic_store(fl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
								if (edge_r)
									__hip_atomic_store(fl + F.ch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							}
					}
				}
				// ---- publish my right half: wait until the previous one has been read, write, bump the counter
				if (it.flags & LW_IF_NEXT_LDS) {
					lds_wait_ge(LW_CNT_ACK(wave), n_pub_used);
					if (two)
						publish<2>(pub, lane, R);
					else
						publish<1>(pub, lane, R);
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					n_pub_used++;
					lds_store_u32(LW_CNT_PUB(wave), n_pub_used);
				}
				// ---- the previous packet's right half: from my predecessor wave through LDS, or (chunk starts) from the
				//      stream's state slot / the halo buffer / a generic predecessor's time-domain block; then window,
				//      overlap-add, conversion and stores, one channel at a time (register pressure)
				if (it.src_kind != LW_SRC_NONE) {
					const float *g = nullptr;
					uint32_t cstride = 0;
					const char *src = nullptr;
					if (it.src_kind == LW_SRC_LDS) {
						++n_got;
						lds_wait_ge(LW_CNT_PUB(wprev), n_got);
						src = pub0 + wprev * LW_PUB_BYTES;
					} else if (it.src_kind == LW_SRC_STATE) {
						const uint32_t pin = (it.flags & LW_RF_PARITY_IN) ? 1u : 0u;
						g = F.state + ((size_t)it.src_arg * 2 + pin) * F.state_stride;
						cstride = F.state_chan_stride;
					} else if (it.src_kind == LW_SRC_HALO) {
						g = F.halo + (size_t)it.src_arg * F.ch * 512u;
						cstride = 512u;
					} else { // LW_SRC_TD: second half of the predecessor's [ch][2048] time-domain block
						g = F.td + (size_t)it.src_arg + 1024u;
						cstride = 2048u;
					}
					if (j == 0)
						LW_STAMP(9);
					if (FMT == LW_OUT_I16_ITL_STEREO) {
						// 2-channel stream decoded as one channel pair: both channels of a sample position leave in one 16-byte store
						uint32_t D[2][4][2];
#pragma unroll
						for (int c = 0; c < 2; c++) {
							PrevHalf ph;
							if (src)
								prev_from_lds(src + 2048 * c, lane, ph);
							else
								prev_from_global(g + (uint32_t)chn[c] * cstride, lane, ph);
							ola_pack_i16(img, lane, R[c], ph, D[c]);
						}
						if (chn[0] == 0)
							store_interleaved2(F, lane, it.out_off, D[0], D[1]);
						else
							store_interleaved2(F, lane, it.out_off, D[1], D[0]);
					} else if (FMT == LW_OUT_F32_ITL_STEREO) {
						// the same for f32: a lane's four positions of both channels are 32 contiguous bytes
						float4_t V[2][4];
#pragma unroll
						for (int c = 0; c < 2; c++) {
							PrevHalf ph;
							if (src)
								prev_from_lds(src + 2048 * c, lane, ph);
							else
								prev_from_global(g + (uint32_t)chn[c] * cstride, lane, ph);
							ola_quads_f32(img, lane, R[c], ph, V[c]);
						}
						if (chn[0] == 0)
							store_interleaved2_f32(F, lane, it.out_off, V[0], V[1]);
						else
							store_interleaved2_f32(F, lane, it.out_off, V[1], V[0]);
					} else {
#pragma unroll
						for (int c = 0; c < 2; c++)
							if (c == 0 || two) {
								PrevHalf ph;
								if (src)
									prev_from_lds(src + 2048 * c, lane, ph);
								else
									prev_from_global(g + (uint32_t)chn[c] * cstride, lane, ph);
								ola_store<FMT>(F, img, lane, chn[c], it.out_off, R[c], ph, e_m);
							}
					}
					if (src) {
						asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
						lds_store_u32(LW_CNT_ACK(wprev), n_got);
					}
				}
				if (EDGE && (edge_l || edge_r)) {
					// ---- short slopes: the un-windowed samples past them, the raw edges for k_short, the 128-sample state
#pragma unroll
					for (int c = 0; c < 2; c++)
						if (c == 0 || two) {
							const bool inner = lane >= 16u; // this lane's q in [508 - 4 lane, +4) lies below 448
							const bool sound = !(it.flags & LW_IF_SILENT); // (the first packet of a stream yields no samples at all)
							float *edge = F.edge + ((size_t)it.pkt * 2u * F.ch + (uint32_t)chn[c]) * LW_EDGE_VALUES;
							if (edge_l) {
								// cur[1023 - q] = -pa(q) for q < 448 (imdct.rs:589-658), positions 576..1023 -> samples 128..575
								const float4_t lo0 = LW_PA_LO0(c), lo1 = LW_PA_LO1(c);
								store_quad<FMT>(F, chn[c], it.out_off, e_m, 1020u - 4u * lane - 448u, float4_t{-lo0.w, -lo0.z, -lo0.y, -lo0.x}, sound);
								store_quad<FMT>(F, chn[c], it.out_off, e_m, 512u + 4u * lane - 448u, float4_t{-lo1.w, -lo1.z, -lo1.y, -lo1.x}, sound && inner);
								if (!inner && !MIXF) // raw left edge pa(448 + i), i = 60 - 4 lane ..
									store16_wt(edge + 60u - 4u * lane, lo1);
							}
							if (edge_r) {
								// cur[1024 + q] = pb(q) for q < 448: positions 1024..1471
								const float4_t lo0 = LW_PB_LO0(c), lo1 = LW_PB_LO1(c);
								store_quad<FMT>(F, chn[c], it.out_off, e_m, 1024u + 4u * lane - e_ls, lo0, sound);
								store_quad<FMT>(F, chn[c], it.out_off, e_m, 1532u - 4u * lane - e_ls, lo1, sound && inner);
								if (!inner) { // raw right part cur[1472 .. 1600): pb(448 + i), then mirrored
									if (!MIXF)
										store16_wt(edge + (size_t)F.ch * LW_EDGE_VALUES + 60u - 4u * lane, lo1);
									if (it.state_out >= 0) {
										float *dst = F.state + ((size_t)it.state_out * 2 + ((it.flags & LW_RF_PARITY_OUT) ? 1u : 0u)) * F.state_stride +
											(uint32_t)chn[c] * F.state_chan_stride;
										store16_wt(dst + 60u - 4u * lane, lo1);
										store16_wt(dst + 64u + 4u * lane, float4_t{lo1.w, lo1.z, lo1.y, lo1.x});
									}
								}
							}
						}
				}
				// ---- raw right half to the stream's state slot and/or to the td block a generic successor reads
				const bool to_state = it.state_out >= 0 && !edge_r, to_td = (it.flags & LW_RF_WRITE_TD) != 0;
				if (to_state || to_td) {
#pragma unroll
					for (int c = 0; c < 2; c++)
						if (c == 0 || two) {
							const float4_t lo0 = LW_PB_LO0(c), lo1 = LW_PB_LO1(c);
							if (to_state) {
								const uint32_t pout = (it.flags & LW_RF_PARITY_OUT) ? 1u : 0u;
								store_right_half(F.state + ((size_t)it.state_out * 2 + pout) * F.state_stride +
										(uint32_t)chn[c] * F.state_chan_stride, lane, lo0, lo1);
							}
							if (to_td)
								store_right_half(F.td + 2u * (size_t)it.res_off + (uint32_t)chn[c] * 2048u + 1024u, lane, lo0, lo1);
							if (TD && (it.flags & LW_IF_TDONLY)) // the un-windowed left half too: cur[q] = pa(q), cur[1023 - q] = -pa(q)
								store_left_half(F.td + 2u * (size_t)it.res_off + (uint32_t)chn[c] * 2048u, lane, LW_PA_LO0(c), LW_PA_LO1(c));
						}
				}
			}
		}
		if (j == 0)
			LW_STAMP(10);
		__builtin_amdgcn_s_setprio(0);
		// ---- HBM loads of the next round
		if (valid_n) {
			if (F.dense) {
				dense_offsets(F, item_n, itn);
				issue_loads<!PRE>(F, itn, un, lane, pf);
				if (PRE)
					issue_pre_loads(F, itn, pre_prog, lane, pq);
				itn = load_item(F.items, item_n);
			} else {
				issue_loads<!PRE>(F, itn, un, lane, pf);
				if (PRE)
					issue_pre_loads(F, itn, pre_prog, lane, pq);
			}
			// ... and its spectrum (waits for them; the stage sits here, not at the top of the loop, so that round 0 can
			// enter the loop with its spectrum already built on either of the two paths above)
			if (PRE)
				apply_pre(pre_prog, pf, pq);
			if (two)
				spectrum_fused<2>(F, img, sc, lane, un, pf);
			else
				spectrum_fused<1, SPLIT>(F, img, sc, lane, un, pf);
		}
		it = itn;
		valid = valid_n;
	}
	LW_STAMP_W(11);
	LW_STAMP_FLUSH;
