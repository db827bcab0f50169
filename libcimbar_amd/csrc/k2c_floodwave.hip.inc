// k2c_floodwave.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K2c: the flood pass for frames whose outcome does not depend on the reference's tie-breaking -- a batch-parallel replacement for
// most of the exact replay (K2b), with a proof obligation checked on the fly; anything it cannot certify is left to K2b.
// ------------------------------------------------------------------------------------------------ K2c confluent flood
// FloodDecodePositions (FloodDecodePositions.cpp:49-134) is Prim's algorithm: "decode SOME cell whose best offered priority is minimal",
// where libstdc++'s heap only decides WHICH of several tied cells goes first; a cell's input (drift, cooldown) is the best offer made
// to it before it is decoded, the first one among equals. This kernel
//   1. replays the first FW_PREFIX cells exactly (one wavefront, the K2b step: real heap, real tie order -- the first cells of a shifted
//      frame are decoded from garbage and genuinely depend on that order), then
//   2. continues in "super-rounds": p = the minimal priority among the cells still to decode; all cells tied at p, and every cell that
//      joins them through an offer of priority p, are decoded as ONE batch, 256 at a time, in any order -- while checking that no order
//      the reference could have taken would have handed any cell a different input:
//        B1  two offers of equal priority but different content reach a cell within one super-round            (first one wins: order)
//        B2  a member's own distance d is below p although it is not the only cell of its super-round (its cheaper offers could
//            overtake a tied cell)
//        B3  a member's offer is better than the input another member of the same super-round was / will be decoded with
//        B4  ... or ties with it (that input stemming from this super-round) with a different content
//      If none fires, every schedule gives every cell the same input, so the batch result IS the reference's (symbols and drifted
//      positions). If one fires the frame keeps flood_flag == 1 and K2b replays it exactly.
// oracle/flood_model.c is the CPU model of exactly these rules; tests/test_flood_model.py checks its claim ("certified => equal to
// the reference's flood") on distorted frames, tests/test_gpu_flood.py checks this kernel against the oracle.
// Clean frames that are merely shifted / partly wiped certify (after the prefix everything rides one priority-0 wave); noisy and
// resampled frames, whose priorities are mixed everywhere, do not.
constexpr int FW_PREFIX = 64;            // cells decoded by the exact replay first
constexpr int FW_HEAP = 1024;            // 8 seeds + 64 * 12 offers at most
constexpr int FW_MAX_ROUNDS = 64;        // certified frames need a handful; a frame that fragments into many tiny rounds is K2b's
// (FW_GRID, the workgroups of a launch -- 75 KiB of LDS each, two per CU: chainplan.hip.inc)
constexpr int FW_BITWORDS = (NCELLS + 31) / 32;
static_assert(FW_HEAP >= 8 + 12 * FW_PREFIX + 16, "the prefix must never reach the spill half of the heap");

// FloodDecodePositions.cpp:27-41: the priority of a cell's seed entry, 0xFE if it has none
__device__ __forceinline__ uint32_t seed_prio_of(int i)
{
	const int s = seed_slot(i);
	return s < 0 ? 0xFEu : (s < 4 ? 0u : 1u);
}
__device__ __forceinline__ int seed_cell_of(int slot)
{
	const int last = NCELLS - 1;
	switch (slot) {
		case 0: return 0;
		case 1: return TOP_W - 1;
		case 2: return last;
		case 3: return last - (TOP_W - 1);
		case 4: return TOP_CELLS;
		case 5: return TOP_CELLS + DIM_X - 1;
		case 6: return last - TOP_CELLS;
		default: return last - (TOP_CELLS + DIM_X - 1);
	}
}

struct FwOut { uint32_t sym, w, dist; };
// CimbReader::read's decode_symbol for one cell on one lane (CimbDecoder.cpp:101-147): window rows from the bit plane, the visiting
// order 4,5,7,3,1,(8,0,2,6), the cooldown skip, strict minimum, stop at the first distance 0
__device__ __forceinline__ FwOut fw_decode(const uint32_t* __restrict__ pl, int cell, int ddx, int ddy, uint32_t cooldown)
{
	int cx, cy;
	if (cell < TOP_CELLS) { cx = OFFSET + (MARKER + cell % TOP_W) * PITCH; cy = OFFSET + (cell / TOP_W) * PITCH; }
	else if (cell < TOP_CELLS + MID_CELLS) { const int q = cell - TOP_CELLS; cx = OFFSET + (q % DIM_X) * PITCH; cy = OFFSET + (MARKER + q / DIM_X) * PITCH; }
	else { const int q = cell - TOP_CELLS - MID_CELLS; cx = OFFSET + (MARKER + q % TOP_W) * PITCH; cy = OFFSET + (DIM_Y - MARKER + q / TOP_W) * PITCH; }
	uint32_t rows[10];
	window_rows(pl, cx + ddx - 1, cy + ddy - 1, rows);
	FwOut o;
	const uint32_t ex = exact_tile(window_hash(rows, 4));
	if (ex < 16u) { o.sym = ex; o.w = 4; o.dist = 0; return o; }
	const int nwin = cooldown == 0xFEu ? 9 : 5;
	uint32_t best = 0xFFFFFFFFu;
	for (int k = 0; k < nwin; ++k) {
		const uint32_t w = k < 8 ? (FLOOD_ORDER8 >> (4 * k)) & 15u : 6u;
		if (w == cooldown && w != 4u) continue;
		const uint32_t bt = best_tile(window_hash(rows, (int)w));          // dist << 4 | tile, first minimum
		const uint32_t key = ((bt >> 4) << 8) | ((uint32_t)k << 4) | (bt & 15u);
		best = key < best ? key : best;
		if ((bt >> 4) == 0u) break;
	}
	const uint32_t kbest = (best >> 4) & 15u;
	o.sym = best & 15u;
	o.w = kbest < 8 ? (FLOOD_ORDER8 >> (4 * kbest)) & 15u : 6u;
	o.dist = best >> 8;
	return o;
}

__device__ __forceinline__ bool fw_bit(const uint32_t* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; }
// returns the bit's previous value
__device__ __forceinline__ bool fw_set(uint32_t* bits, int i) { return (atomicOr(&bits[i >> 5], 1u << (i & 31)) >> (i & 31)) & 1u; }

__global__ __launch_bounds__(256) void k_flood_wave(const uint32_t* __restrict__ plane, Tables tb, uint32_t* __restrict__ queues,
                                                    uint32_t* __restrict__ flood_flag, uint8_t* __restrict__ symbols,
                                                    int8_t* __restrict__ drift, int f0, int nframes, int area0, uint32_t* __restrict__ info)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_state[NCELLS + 16];   // prefix: as in k_flood; batch phase: 0x80 | symbol once decoded, else 0
	__shared__ uint32_t s_heap[FW_HEAP];
	__shared__ uint32_t s_seed[8];
	__shared__ uint32_t s_cell[NCELLS];             // best offer so far: priority << 16 | content (dx+8 << 7 | dy+8 << 3 | cooldown code); priority 0xFE = none
	__shared__ uint32_t s_cur[FW_BITWORDS];         // that offer was made in the current super-round
	__shared__ uint32_t s_member[FW_BITWORDS];      // the cell belongs to the current super-round (queued, decoded or not)
	__shared__ int s_tail, s_bail, s_hn, s_red[4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t* queue = queues + (size_t)(area0 + blockIdx.x) * NCELLS;

	for (int fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
		const int f = f0 + fi;
		if (flood_flag[f] != 1u) continue;
		const uint32_t* pl = plane + (size_t)f * PLANE_WORDS;
		int8_t* drift_frame = drift + (size_t)f * NCELLS * 2;
		__syncthreads();   // the previous frame of this workgroup is done with the LDS

		// ---- 1. exact prefix, wavefront 0
		if (wave == 0) {
			WaveHeap<FW_HEAP> hp{(lds_u32*)s_heap, nullptr, 0};
			hp.lanes(lane);
			flood_reset(hp, s_state, s_seed, lane, 64);
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_s_waitcnt(0);
			flood_seed(hp, lane);
			const FloodLane fl = flood_lane_init(lane);
#ifdef FLOOD_PROF
			unsigned long long pt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
			for (int count = 0; count < FW_PREFIX; ++count) {
#ifdef FLOOD_PROF
				if (!flood_step<false>(hp, s_state, s_seed, pl, tb, drift_frame, fl, pt)) break;
#else
				if (!flood_step<false>(hp, s_state, s_seed, pl, tb, drift_frame, fl)) break;
#endif
			}
			if (lane == 0) { s_hn = hp.n; s_bail = 0; }
		}
		__syncthreads();

		// ---- 2. hand-over: per-cell best offer out of the heap entries (the entry whose priority is the cell's best IS its latest
		// instruction; seeds keep theirs in s_seed), visited flags re-encoded
		for (int c = tid; c < NCELLS; c += 256) s_cell[c] = (0xFEu << 16) | FLOOD_DEFAULT_D;
		__syncthreads();
		for (int k = tid; k < s_hn; k += 256) {
			const uint32_t e = s_heap[k];
			const int cell = (int)((e >> 11) & 0x3FFFu);
			const uint32_t st = s_state[cell];
			if (!(st & 0x80u) && st == (e >> 25) + 1u && seed_slot(cell) < 0) s_cell[cell] = ((e >> 25) << 16) | (e & 0x7FFu);
		}
		if (tid < 8) {
			const int cell = seed_cell_of(tid);
			const uint32_t sv = s_seed[tid];
			if (!(s_state[cell] & 0x80u) && (sv >> 16) != 0xFEu) s_cell[cell] = sv;   // same layout: priority << 16 | content
		}
		__syncthreads();
		for (int c = tid; c < NCELLS; c += 256) { const uint32_t st = s_state[c]; s_state[c] = (st & 0x80u) ? (uint8_t)st : (uint8_t)0; }
		__syncthreads();

		// ---- 3. super-rounds
		bool certified = false;
		int round = 0;
		for (; round < FW_MAX_ROUNDS; ++round) {
			// p = the cheapest cell still to decode (its seed entry or its best offer, whichever pops first)
			uint32_t pmin = 0xFEu;
			for (int c = tid; c < NCELLS; c += 256)
				if (!(s_state[c] & 0x80u)) {
					const uint32_t q = min(seed_prio_of(c), s_cell[c] >> 16);
					pmin = q < pmin ? q : pmin;
				}
			pmin = wave_min(pmin);
			if (lane == 0) s_red[wave] = (int)pmin;
			for (int k = tid; k < FW_BITWORDS; k += 256) { s_cur[k] = 0; s_member[k] = 0; }
			if (tid == 0) s_tail = 0;
			__syncthreads();
			const uint32_t p = (uint32_t)min(min(s_red[0], s_red[1]), min(s_red[2], s_red[3]));
			if (p == 0xFEu) { certified = true; break; }   // nothing left that can be reached (as in the reference, the rest stays undecoded)
			for (int c = tid; c < NCELLS; c += 256)
				if (!(s_state[c] & 0x80u) && min(seed_prio_of(c), s_cell[c] >> 16) == p) {
					const int pos = atomicAdd(&s_tail, 1);
					__hip_atomic_store(&queue[pos], (uint32_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					fw_set(s_member, c);
				}
			__syncthreads();
			const int tied = s_tail;
			int head = 0;
			while (head < s_tail) {
				const int tail = s_tail;
				const int chunk = min(256, tail - head);
				const bool sole = tied == 1 && head == 0 && tail == 1;
				// pass 1a: decode one member per lane; snapshot what its targets hold BEFORE this chunk's offers
				int m = -1, nprop = 0, ntgt = 0;
				uint32_t mykey = 0, dist = 0, nk = 0;
				int16_t tgt[12], prop[12];
				uint32_t snap[12];
				if (tid < chunk) {
					m = (int)__hip_atomic_load(&queue[head + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					const uint32_t cv = s_cell[m];
					const uint32_t din = cv >> 16, content = cv & 0x7FFu;
					const int ddx = (int)(content >> 7) - 8, ddy = (int)((content >> 3) & 15u) - 8;
					const uint32_t cooldown = cool_dec(content & 7u);
					const FwOut o = fw_decode(pl, m, ddx, ddy, cooldown);
					dist = o.dist;
					if (dist < p && !sole) s_bail = 2;
					const int bdx = (int)(o.w % 3) - 1, bdy = (int)(o.w / 3) - 1;
					int ndx = ddx + bdx, ndy = ddy + bdy;
					ndx = ndx > 7 ? 7 : (ndx < -7 ? -7 : ndx);
					ndy = ndy > 7 ? 7 : (ndy < -7 ? -7 : ndy);
					const uint32_t ncool = calc_cooldown(cooldown, o.w);
					s_state[m] = (uint8_t)(0x80u | o.sym);
					*reinterpret_cast<uint16_t*>(drift_frame + (size_t)m * 2) =
					    (uint16_t)(((uint32_t)(ddx + bdx) & 0xFFu) | (((uint32_t)(ddy + bdy) & 0xFFu) << 8));
					const bool far = din < 3u && dist < 3u && cooldown == 4u && ncool == 4u;
					nk = ((uint32_t)(ndx + 8) << 7) | ((uint32_t)(ndy + 8) << 3) | cool_enc(ncool);
					mykey = (dist << 16) | nk;
					const int16_t* cand = tb.cand + (size_t)m * 12;
					const int nq = far ? 12 : 4;
					for (int q = 0; q < nq; ++q) {
						const int t = cand[q];
						if (t < 0) continue;
						tgt[ntgt] = (int16_t)t;
						snap[ntgt++] = s_cell[t];
					}
				}
				__syncthreads();
				// pass 1b: check the offers against the other members of the super-round, propose the rest
				for (int q = 0; q < ntgt; ++q) {
					const int t = tgt[q];
					const uint32_t tv = snap[q], td = tv >> 16;
					if (fw_bit(s_member, t)) {
						// another cell of this super-round: some schedule decodes it after this one
						if (dist < td) s_bail = 3;
						else if (dist == td && fw_bit(s_cur, t) && nk != (tv & 0x7FFu)) s_bail = 4;
						continue;
					}
					if (s_state[t] & 0x80u) continue;                  // decoded in an earlier super-round, in every schedule
					if (dist < td) { atomicMin(&s_cell[t], mykey); prop[nprop++] = (int16_t)t; }
					else if (dist == td && fw_bit(s_cur, t) && nk != (tv & 0x7FFu)) s_bail = 1;   // equal priority, other content, earlier chunk
				}
				__syncthreads();
				// pass 2: an offer that is now the cell's best: the cell joins the super-round if its priority is p
				for (int q = 0; q < nprop; ++q) {
					const int t = prop[q];
					const uint32_t v = s_cell[t];
					if ((v >> 16) != dist) continue;                       // a better offer of this chunk won
					if (v != mykey) { s_bail = 1; continue; }              // equal priority, different content, same chunk
					fw_set(s_cur, t);
					if (dist == p && !fw_set(s_member, t)) {
						const int pos = atomicAdd(&s_tail, 1);
						__hip_atomic_store(&queue[pos], (uint32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					}
				}
				__syncthreads();
				head += chunk;
				if (s_bail) break;
			}
			if (s_bail) break;
		}
		__syncthreads();
		// what happened, for CIMBAR_HIP_TAP_FLOOD_INFO: rule that declined the frame (0 = certified, 1..4 = B1..B4, 5 = out of super-rounds) |
		// the super-round it happened in << 8 | cells decoded by then << 16
		{
			int done = 0;
			for (int c = tid; c < NCELLS; c += 256) done += (s_state[c] & 0x80u) ? 1 : 0;
			for (int o = 32; o > 0; o >>= 1) done += __shfl_down(done, o);
			if (lane == 0) s_red[wave] = done;
			__syncthreads();
			if (tid == 0) info[f] = (uint32_t)(s_bail ? s_bail : (certified ? 0 : 5)) | ((uint32_t)round << 8) | ((uint32_t)(s_red[0] + s_red[1] + s_red[2] + s_red[3]) << 16);
			__syncthreads();
		}
		if (certified && !s_bail) {
			for (int c = tid; c < NCELLS; c += 256) {
				const uint32_t v = s_state[c];
				if (v & 0x80u) symbols[(size_t)f * NCELLS + c] = (uint8_t)(v & 15u);
			}
			if (tid == 0) flood_flag[f] = 2u;
		}
	}
}

// ---- CIMBAR_HIP_FLOOD_VERIFY: the certificate checked against the exact replay, frame by frame ---------------------------------------
// k_verify_begin sets the results of every frame k_flood_wave certified (flag 2) aside and flags exactly those frames for the exact kernel;
// k_verify_end compares what the exact replay made of them: vflag[cap + f] = cells whose symbol or drifted position differ (0xFFFFFFFF for a
// frame that was not certified), totals[0] += frames compared, totals[1] += frames that differed.
__global__ __launch_bounds__(256) void k_verify_begin(const uint32_t* __restrict__ flood_flag, const uint8_t* __restrict__ symbols, const int8_t* __restrict__ drift,
                                                      uint32_t* __restrict__ vflag, uint8_t* __restrict__ vsym, int8_t* __restrict__ vdrift, int f0, int cap)
{
	const int f = f0 + blockIdx.x;
	const bool certified = flood_flag[f] == 2u;
	if (threadIdx.x == 0) { vflag[f] = certified ? 1u : 0u; vflag[cap + f] = certified ? 0u : 0xFFFFFFFFu; }
	if (!certified) return;
	const uint32_t* s4 = reinterpret_cast<const uint32_t*>(symbols + (size_t)f * NCELLS);
	uint32_t* d4 = reinterpret_cast<uint32_t*>(vsym + (size_t)f * NCELLS);
	for (int i = threadIdx.x; i < NCELLS / 4; i += 256) d4[i] = s4[i];
	const uint32_t* s2 = reinterpret_cast<const uint32_t*>(drift + (size_t)f * NCELLS * 2);
	uint32_t* d2 = reinterpret_cast<uint32_t*>(vdrift + (size_t)f * NCELLS * 2);
	for (int i = threadIdx.x; i < NCELLS / 2; i += 256) d2[i] = s2[i];
}
static_assert(NCELLS % 4 == 0, "k_verify_* copy whole dwords");
__global__ __launch_bounds__(256) void k_verify_end(const uint8_t* __restrict__ symbols, const int8_t* __restrict__ drift, uint32_t* __restrict__ vflag,
                                                    const uint8_t* __restrict__ vsym, const int8_t* __restrict__ vdrift, int f0, int cap, unsigned long long* __restrict__ totals)
{
	const int f = f0 + blockIdx.x;
	if (vflag[f] != 1u) return;
	__shared__ uint32_t s_bad;
	if (threadIdx.x == 0) s_bad = 0;
	__syncthreads();
	uint32_t bad = 0;
	for (int i = threadIdx.x; i < NCELLS; i += 256) {
		const size_t c = (size_t)f * NCELLS + i;
		bad += (symbols[c] != vsym[c] || drift[2 * c] != vdrift[2 * c] || drift[2 * c + 1] != vdrift[2 * c + 1]) ? 1u : 0u;
	}
	if (bad) atomicAdd(&s_bad, bad);
	__syncthreads();
	if (threadIdx.x == 0) {
		vflag[cap + f] = s_bad;
		atomicAdd(&totals[0], 1ull);
		if (s_bad) atomicAdd(&totals[1], 1ull);
	}
}

// how many frames of the batch left the parallel pass (flag 1 or 2) and how many of those the certifying pass did not settle (flag 1 or 3), into pinned host
// memory: inputs of enqueue()'s scheduling decisions ("split the chain or not", "is the certifying pass worth running")
__global__ __launch_bounds__(256) void k_count_flagged(const uint32_t* __restrict__ flood_flag, int n, uint32_t* __restrict__ host_out)
{
	__shared__ uint32_t s_n, s_x;
	if (threadIdx.x == 0) { s_n = 0; s_x = 0; }
	__syncthreads();
	uint32_t c = 0, x = 0;
	for (int f = threadIdx.x; f < n; f += 256) { const uint32_t fl = flood_flag[f]; c += fl != 0u ? 1u : 0u; x += (fl == 1u || fl == 3u) ? 1u : 0u; }   // (3: flooded in rounds -- not certified either)
	if (c) atomicAdd(&s_n, c);
	if (x) atomicAdd(&s_x, x);
	__syncthreads();
	if (threadIdx.x == 0) { host_out[0] = s_n; host_out[1] = (uint32_t)n; host_out[2] = s_x; }
}
