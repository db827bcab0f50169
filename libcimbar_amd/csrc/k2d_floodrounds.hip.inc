// k2d_floodrounds.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K2d: the relaxed flood -- threshold rounds (opt-in: cimbar_hip_set_relaxed_flood; DESIGN_WIDENING.md "Relaxed flood")
// ------------------------------------------------------------------------------------------------ K2d relaxed flood
// The exact replay (K2b) keeps the ORDER in which the reference's heap hands out cells, 12 400 dependent steps per frame. This pass keeps the
// reference's rule -- a cell is decoded at the drift of its most confident neighbour, cells offered by confident neighbours go first -- and
// drops the tie order, so that a frame is flooded in 40 .. 1 000 parallel rounds. Its result is NOT the reference's cell for cell; the chain
// accepts it per frame only where every symbol RS block decodes (k_rounds_check) and hands everything else to the exact replay.
//
// The rule, per flagged frame (tests/relaxed_flood_model.py is its numpy restatement, tests/test_gpu_relaxed_flood.py holds the two together):
//   * a cell is decoded exactly as K2b decodes it (fw_decode: window at cell + drift - 1, nine or five windows by cooldown, best_symbol's
//     visiting order and first minimum, new drift clamped to +-7, calc_cooldown);
//   * a decoded cell with distance d offers (d, its new drift, its new cooldown) to its four adjacent cells, and to the eight horizon cells
//     under FloodDecodePositions::update's condition (input priority < 3, d < 3, input and new cooldown 4); tb.cand is the offer list with the
//     list's own preconditions folded in. Decoded cells take no offers;
//   * a cell's input is the offer with the smallest (priority, offering cell) it has received: one u32 key per cell in LDS,
//         priority(7) << 25 | offering cell + 1 (14) << 11 | dx+8 (4) << 7 | dy+8 (4) << 3 | cooldown code (3)
//     -- K2b's heap entry with the offerer where the cell was -- so that an offer is one LDS atomicMin and the order in which a round's lanes
//     make their offers cannot matter. The seeds start with the reference's seed offers, offering cell field 0 = "before every cell";
//   * a round: pmin = the smallest input priority among the offered, undecoded cells (none: the frame is done); T = max(threshold, pmin); every
//     such cell whose input priority is <= T is decoded from its input as it stands at the round's start; then all of them make their offers.
// Every round decodes at least one cell, so there are at most NCELLS rounds; the round loop carries that bound as a hard counter.
//
// One workgroup per frame, persistent over a strided frame list like k_flood_wave. Per round: the OPEN list (offered, undecoded cells) is read
// twice -- the minimum, then the split into this round's members and the cells that stay open -- and the members are then decoded one per lane.
// A member's "frozen" bit is set before any offer of the round is made: offers skip frozen cells, which is what keeps a member's input as it
// stood at the round's start however many passes of 512 lanes the round takes. The open list is double-buffered: the cells that stay open and
// the cells that receive their first offer are appended to the other buffer, whose far end holds the round's members meanwhile (members, open
// and newly offered cells are distinct undecoded cells, so the two ends cannot meet).
// LDS: 49 600 (keys) + 2 x 24 800 (lists) + 1 552 (bits) = 100.8 KB in mode 68 -- one workgroup of eight wavefronts per CU (69.8 KB in mode 67:
// two, 43.7 KB in mode 66: three). Synchronisation is workgroup barriers only; nothing here reads memory another workgroup writes.
constexpr int FR_THREADS = 512;
constexpr int FR_LDS = NCELLS * 4 + 2 * NCELLS * 2 + FW_BITWORDS * 4 + 16;
constexpr int FR_GRID = 256 * (160 * 1024 / FR_LDS);   // as many workgroups as the chip holds at once (CIMBAR_HIP_ROUNDS_GRID lowers it: cimbar_hip_create)
static_assert(FR_LDS <= 160 * 1024 && FR_GRID * FR_THREADS <= 256 * 2048, "a workgroup fits a CU");
constexpr uint32_t FR_NONE = 0xFFFFFFFFu;
constexpr int FR_THRESHOLD_MAX = 32;
static_assert(NCELLS + 1 < (1 << 14), "the offering cell + 1 fits the key's 14 bits");

__global__ __launch_bounds__(FR_THREADS) void k_flood_rounds(const uint32_t* __restrict__ plane, Tables tb, uint32_t* __restrict__ flood_flag,
                                                             uint8_t* __restrict__ symbols, int8_t* __restrict__ drift, int f0, int nframes,
                                                             uint32_t threshold, uint32_t* __restrict__ info)
{
	__shared__ uint32_t s_key[NCELLS];              // best offer so far (the cell's input once it is decoded); FR_NONE = no offer yet
	__shared__ uint16_t s_list[2][NCELLS];          // open list, double-buffered; the far end of the buffer being filled holds the round's members
	__shared__ uint32_t s_frozen[FW_BITWORDS];      // the cell is decoded, or is being decoded in this round: it takes no offers
	__shared__ uint32_t s_n[2], s_members, s_pmin;
	const int tid = threadIdx.x, lane = tid & 63;

	for (int fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
		const int f = f0 + fi;
		if (flood_flag[f] != 1u) continue;
		const uint32_t* pl = plane + (size_t)f * PLANE_WORDS;
		uint8_t* sym_frame = symbols + (size_t)f * NCELLS;
		int8_t* drift_frame = drift + (size_t)f * NCELLS * 2;
		__syncthreads();   // the previous frame of this workgroup is done with the LDS

		for (int c = tid; c < NCELLS; c += FR_THREADS) s_key[c] = FR_NONE;
		for (int k = tid; k < FW_BITWORDS; k += FR_THREADS) s_frozen[k] = 0;
		__syncthreads();
		if (tid < 8) {
			// FloodDecodePositions.cpp:27-41: the seed offers (priority 0 | 1, drift (0,0), cooldown 0xFE), from "before every cell"
			const int cell = seed_cell_of(tid);
			s_key[cell] = ((tid < 4 ? 0u : 1u) << 25) | FLOOD_DEFAULT_D;
			s_list[0][tid] = (uint16_t)cell;
		}
		if (tid == 0) { s_n[0] = 8; s_n[1] = 0; s_members = 0; s_pmin = 0xFFu; }
		__syncthreads();

		uint32_t rounds = 0, decoded = 0;
		for (int a = 0; rounds < (uint32_t)NCELLS; a ^= 1) {
			const int b = a ^ 1;
			const int n = (int)s_n[a];
			if (n == 0) break;
			const uint16_t* open = s_list[a];
			uint16_t* next = s_list[b];
			// ---- the smallest input priority among the open cells
			{
				uint32_t p = 0xFFu;
				for (int k = tid; k < n; k += FR_THREADS) { const uint32_t q = s_key[open[k]] >> 25; p = q < p ? q : p; }
				p = wave_min(p);
				if (lane == 0) atomicMin(&s_pmin, p);
				// (the last round's member count: every lane read it before that round's closing barrier, and nothing adds to it before the barrier below)
				if (tid == 0) s_members = 0;
			}
			__syncthreads();
			const uint32_t pmin = s_pmin;
			const uint32_t T = threshold > pmin ? threshold : pmin;
			// ---- members (frozen from here on) to the far end of the other buffer, everything else stays open
			for (int k = tid; k < n; k += FR_THREADS) {
				const int c = open[k];
				if ((s_key[c] >> 25) <= T) {
					fw_set(s_frozen, c);
					next[NCELLS - 1 - (int)atomicAdd(&s_members, 1u)] = (uint16_t)c;
				} else next[atomicAdd(&s_n[b], 1u)] = (uint16_t)c;
			}
			__syncthreads();
			const int members = (int)s_members;
			// ---- decode the members from their inputs, one per lane; then their offers (a member's own key is read by its lane alone, and no
			// offer reaches a frozen cell: whatever pass of FR_THREADS a member falls into, it sees its input as it stood at the round's start)
			for (int k = tid; k < members; k += FR_THREADS) {
				const int m = next[NCELLS - 1 - k];
				const uint32_t key = s_key[m];
				const uint32_t din = ((key >> 11) & 0x3FFFu) ? key >> 25 : 0xFEu;   // (a seed decoded from its own seed offer: FloodDecodePositions' instruction still says 0xFE)
				const int ddx = (int)((key >> 7) & 15u) - 8, ddy = (int)((key >> 3) & 15u) - 8;
				const uint32_t cooldown = cool_dec(key & 7u);
				const FwOut o = fw_decode(pl, m, ddx, ddy, cooldown);
				const int bdx = (int)(o.w % 3) - 1, bdy = (int)(o.w / 3) - 1;
				int ndx = ddx + bdx, ndy = ddy + bdy;
				ndx = ndx > 7 ? 7 : (ndx < -7 ? -7 : ndx);
				ndy = ndy > 7 ? 7 : (ndy < -7 ? -7 : ndy);
				const uint32_t ncool = calc_cooldown(cooldown, o.w);
				sym_frame[m] = (uint8_t)o.sym;
				*reinterpret_cast<uint16_t*>(drift_frame + (size_t)m * 2) =
				    (uint16_t)(((uint32_t)(ddx + bdx) & 0xFFu) | (((uint32_t)(ddy + bdy) & 0xFFu) << 8));
				const bool far = din < 3u && o.dist < 3u && cooldown == 4u && ncool == 4u;
				const uint32_t offer = (o.dist << 25) | ((uint32_t)(m + 1) << 11) | ((uint32_t)(ndx + 8) << 7) | ((uint32_t)(ndy + 8) << 3) | cool_enc(ncool);
				const int16_t* cand = tb.cand + (size_t)m * 12;
				const int nq = far ? 12 : 4;
				for (int q = 0; q < nq; ++q) {
					const int t = cand[q];
					if (t < 0 || fw_bit(s_frozen, t)) continue;
					if (atomicMin(&s_key[t], offer) == FR_NONE) next[atomicAdd(&s_n[b], 1u)] = (uint16_t)t;   // its first offer: the cell is open now
				}
			}
			decoded += (uint32_t)members;
			++rounds;
			// (every lane read s_n[a] before this round's first barrier and s_pmin before its second. s_members was read BEHIND the second: it is reset at the
			// top of the next round, where this round's closing barrier lies in between)
			if (tid == 0) { s_n[a] = 0; s_pmin = 0xFFu; }
			__syncthreads();
		}
		// flooded in rounds; CIMBAR_HIP_TAP_FLOOD_ROUNDS: rounds | cells decoded << 16
		if (tid == 0) { flood_flag[f] = 3u; info[f] = rounds | (decoded << 16); }
	}
}

// The acceptance test of the relaxed flood, behind the symbol streams' RS pass: a frame flooded in rounds (flag 3) is accepted iff every one of its
// symbol blocks decoded (each is then a codeword within the correction radius of what the frame showed). With `fallback` a frame that is not goes
// back to flag 1, which is what the exact replay acts on. stats: [0] frames flooded in rounds, [1] accepted, [2] handed to the exact replay,
// [3] rounds in total (cimbar_hip_relaxed_flood_stats).
__global__ __launch_bounds__(256) void k_rounds_check(uint32_t* __restrict__ flood_flag, const uint8_t* __restrict__ rs_ok, const uint32_t* __restrict__ info,
                                                      int f0, int nframes, int fallback, unsigned long long* __restrict__ stats)
{
	const int fi = blockIdx.x * 256 + threadIdx.x;
	if (fi >= nframes) return;
	const int f = f0 + fi;
	if (flood_flag[f] != 3u) return;
	bool ok = true;
	for (int b = 0; b < SYM_BLOCKS; ++b) ok = ok && rs_ok[(size_t)f * ALL_BLOCKS + b] != 0;
	atomicAdd(&stats[0], 1ull);
	atomicAdd(&stats[3], (unsigned long long)(info[f] & 0xFFFFu));
	if (ok) atomicAdd(&stats[1], 1ull);
	else if (fallback) { atomicAdd(&stats[2], 1ull); flood_flag[f] = 1u; }
}
