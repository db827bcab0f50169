// combine.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace, after k4_frame.hip.inc).
// G1-G4: multi-capture decoding -- consecutive captures of one displayed frame decoded once more from the cells of all of them
// ------------------------------------------------------------------------------------------------ grouping and combined cells
// A batch is decoded capture by capture first (enqueue(), unchanged). Then:
//   G1 k_group_agree   agree(k, k+1) = cells whose symbol AND colour are equal in captures k and k+1, one workgroup per pair
//   G2 k_group_walk    one wavefront walks the captures left to right and numbers the runs ("groups"), or takes the caller's numbering; it
//                      writes every group's members (capture indices, ascending, at most GMAX) and the group count to device memory
//   G3 k_group_cells   per group and cell: the combined symbol, colour and margin (the rule below); unanimous cells cost one compare
//   G3c k_group_colour (opt-in, cimbar_hip_set_group_colour_vote) the colour of colour-disputed cells by the members' classifier margins, and
//                      behind G4 k_group_colour_retry, the erasure retry of the colour chunks still missing -- see "colour vote" below
//   K3 k_rs            the same Reed-Solomon kernels as a capture's decode, over the groups' cells (LIVE: workgroups past the count return,
//                      and so does every wavefront of a group whose members agree on every cell -- see k_group_end)
//   G4 k_group_end     the aligned_stream bookkeeping of k_frame_mid + k_frame_end over the group's blocks, the members' chunks for what the
//                      combined decode did not deliver, and (erasure decoding on) the erasure retry of the symbol chunks still missing
// Every kernel after G2 is launched for n captures' worth of groups and returns at once at or above the device-side group count, so nothing
// here waits for the host.
// The plain combined calls' groups do not span calls; the stream calls' (..._combined_stream) do: the group still open at the end of a call is
// kept in a carry store the context owns (at most GMAX - 1 members, copies) and the next stream call walks a virtual batch, the carried
// members followed by its own captures. See "the stream calls" below.
constexpr int GMAX = 8;                    // captures per group at most (the max_group argument is <= this)
constexpr int GROUP_MAX_DEFAULT = 4, GROUP_AGREE_DEFAULT = 750;
constexpr uint16_t MARGIN_NONE = 0xFFFFu;  // the symbol of the cell is not disputed
static_assert(NCELLS % 4 == 0, "a frame's cells are whole dwords");

// the agreeing cells of two captures (symbols s0 / s1, colours c0 / c1, NCELLS bytes each), counted by the whole workgroup
__device__ __forceinline__ uint32_t agreeing_cells(const uint32_t* __restrict__ s0, const uint32_t* __restrict__ c0, const uint32_t* __restrict__ s1,
                                                   const uint32_t* __restrict__ c1)
{
	constexpr int W = NCELLS / 4;
	constexpr uint32_t CM = 0x01010101u * (uint32_t)(NCOLORS - 1);
	uint32_t cnt = 0;
	for (int w = threadIdx.x; w < W; w += 256) {
		const uint32_t x = ((s0[w] ^ s1[w]) & 0x0F0F0F0Fu) | ((c0[w] ^ c1[w]) & CM);
		cnt += ((x & 0xFFu) == 0u) + ((x & 0xFF00u) == 0u) + ((x & 0xFF0000u) == 0u) + ((x >> 24) == 0u);
	}
	for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
	__shared__ uint32_t s_part[4];
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
	__syncthreads();
	return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// G1: one workgroup per pair (k, k+1), k < n - 1
__global__ __launch_bounds__(256) void k_group_agree(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                     uint32_t* __restrict__ agree)
{
	const int k = blockIdx.x;
	if (k + 1 >= n) return;
	const uint32_t* s0 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
	const uint32_t* c0 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
	const uint32_t a = agreeing_cells(s0, c0, s0 + NCELLS / 4, c0 + NCELLS / 4);
	if (threadIdx.x == 0) agree[k] = a;
}

// G2: one wavefront, 64 captures per step, everything carried in registers from step to step.
//  * usable: status == nullptr, or the capture's extraction status > 0
//  * groups_in == nullptr: capture k starts a group when it is usable and it is the first capture, or capture k - 1 is unusable, or
//    agree(k - 1, k) * 1000 < min_agree * NCELLS, or the group before already has max_group members; an unusable capture is in no group
//  * groups_in != nullptr (validated by the host: -1 or ids from 0 rising by one, each id contiguous, at most max_group captures each): the
//    ids as given, except that an unusable capture is left out of its group
// groups[k] = the group of capture k or -1; gmem[g * GMAX + r] = the r-th member of group g; gcount[g] (zeroed by the host) = its members;
// *ngroups = the highest id + 1.
__global__ __launch_bounds__(64) void k_group_walk(const uint32_t* __restrict__ agree, int n, const int* __restrict__ status, int stride,
                                                   const int* __restrict__ groups_in, int min_agree, int max_group, int* __restrict__ groups,
                                                   int* __restrict__ gmem, int* __restrict__ gcount, int* __restrict__ ngroups)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
	int run_carry = 0, starts_carry = 0, mem_carry = 0, base_carry = 0, prev_id = -1, top = -1;
	bool prev_u = false;
	// (each step's loads are issued one step ahead: the walk is otherwise one dependent global load per 64 captures)
	auto fetch = [&](int k, uint32_t& a, int& st, int& gi) {
		a = (!groups_in && k > 0 && k < n) ? agree[k - 1] : 0u;
		st = (status && k < n) ? status[(size_t)k * stride] : 1;
		gi = (groups_in && k < n) ? groups_in[k] : -1;
	};
	uint32_t a_cur; int st_cur, gi_cur;
	fetch(lane, a_cur, st_cur, gi_cur);
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		uint32_t a_nxt; int st_nxt, gi_nxt;
		fetch(k + 64, a_nxt, st_nxt, gi_nxt);
		const bool in = k < n;
		const bool u = in && st_cur > 0;
		const unsigned long long ub = __ballot(u);
		const bool u_prev = lane == 0 ? prev_u : ((ub >> (lane - 1)) & 1ull) != 0;
		int id;
		if (groups_in) id = in ? gi_cur : -1;
		else {
			const bool brk = in && (k == 0 || !u_prev || (unsigned long long)a_cur * 1000ull < (unsigned long long)min_agree * NCELLS);
			const unsigned long long bb = __ballot(brk) & upto;
			const int run = bb ? k0 + 63 - __clzll(bb) : run_carry;          // the latest break at or before k
			const bool start = u && (k - run) % max_group == 0;
			const unsigned long long sb = __ballot(start);
			id = u ? starts_carry + (int)__popcll(sb & upto) - 1 : -1;
			run_carry = __shfl(run, 63);
			starts_carry += (int)__popcll(sb);
		}
		const int id_prev_lane = __shfl(id, lane > 0 ? lane - 1 : 0);
		const int id_prev = lane == 0 ? prev_id : id_prev_lane;
		const bool head = id >= 0 && (k == 0 || id_prev != id);
		const bool member = id >= 0 && u;
		const unsigned long long mb = __ballot(member), hb = __ballot(head) & upto;
		const int before = mem_carry + (int)__popcll(mb & below);           // members of the batch in front of capture k
		const int hl = hb ? 63 - __clzll(hb) : lane;
		const int at_head = __shfl(before, hl);
		const int base = hb ? at_head : base_carry;                          // members in front of k's group
		if (in) groups[k] = member ? id : -1;
		if (member) {
			gmem[(size_t)id * GMAX + (before - base)] = k;
			atomicAdd(&gcount[id], 1);
		}
		top = id > top ? id : top;
		prev_id = __shfl(id, 63);
		prev_u = __shfl((int)u, 63) != 0;
		mem_carry += (int)__popcll(mb);
		base_carry = __shfl(base, 63);
		a_cur = a_nxt; st_cur = st_nxt; gi_cur = gi_nxt;
	}
	for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(top, o); top = t > top ? t : top; }
	if (lane == 0) *ngroups = top + 1;
}

// G3: the combined cells of group blockIdx.y, GC_CELLS cells per workgroup. For cell i with members c (decisions s_c, col_c) and
// d_c(t) = popcount(H_c(i) ^ tile t), H_c(i) = the 8x8 hash of member c's bit plane at its final position (k_erasure_frame's window):
//   symbol  all s_c equal: kept, margin MARGIN_NONE. Otherwise argmin_t sum_c (2 d_c(t) - [t == s_c]), ties to the lowest t; margin = the
//           second-lowest score minus the lowest
//   colour  the plurality of col_c; on a tie, the colour of the member whose colour is among the tied ones and whose d_c(symbol) is smallest,
//           then the lowest member index
// Phase 1 settles every cell whose symbols agree and whose colour vote has one winner (no hash needed); the rest are queued per wavefront
// and phase 2 gives each of them a lane of its own: the cost grows with the disputed cells only.
constexpr int GC_CELLS = 1024, GC_BLOCKS = (NCELLS + GC_CELLS - 1) / GC_CELLS;

// The carry store of the stream calls, by value into their kernels: CARRY_SLOTS members' worth of what G1, G3 and G4 read of a member, and
// the number of occupied slots (always slots 0 .. *count - 1, in capture order). A member id below CARRY_SLOTS names a slot, id - CARRY_SLOTS
// a capture of the call's batch. An unusable capture is in no group, so a slot is a usable capture by construction and holds no status.
constexpr int CARRY_SLOTS = GMAX - 1;
constexpr size_t CS_CELLS = ((size_t)NCELLS + 15) / 16 * 16, CS_DRIFT = ((size_t)NCELLS * 2 + 15) / 16 * 16, CS_PLANE = ((size_t)PLANE_WORDS + 3) / 4 * 4,
                 CS_CHUNKS = ((size_t)FRAME_BYTES + 15) / 16 * 16,   // slot strides (bytes, bytes, words, bytes): every slot starts on 16 bytes
                 CS_WEIGHTS = ((size_t)NCELLS + 3) / 4 * 4;          // (words)
struct CarryStore {
	uint8_t* symbols; uint8_t* colors; uint32_t* plane; int8_t* drift; uint32_t* flood; uint8_t* chunks; uint32_t* masks;
	int* count;
	uint32_t* weights;   // the colour vote's weight of every cell of a member (cimbar_hip_set_stream_colour_vote); nullptr while the stream runs without it
};

// (CARRY = false is the plain calls' kernel as it always was: a member id is a batch index and `cs` is not read. RESCUE, the once-calls' run
// rescue -- k_group_cells_rescue at the end of this file: a member id is a capture index k and rmap[k] says where its cells are, ~slot of
// the rescue store `cs` or, >= 0, a position in the batch pass 2 decoded. SALVAGE, tear salvage -- k_group_cells_salvage at the end of this
// file: RESCUE where a member may take part in some cells only; `in(c)` is "member c takes part in this cell", without SALVAGE c < m)
template <bool CARRY, bool RESCUE = false, bool SALVAGE = false>
__device__ __forceinline__ void group_cells_body(const uint32_t* __restrict__ plane, const Tables& tb, const uint8_t* __restrict__ symbols,
                                                 const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                 const uint32_t* __restrict__ flood_flag, const int* __restrict__ gmem,
                                                 const int* __restrict__ gcount, const int* __restrict__ ngroups, uint8_t* __restrict__ gsym,
                                                 uint8_t* __restrict__ gcol, uint16_t* __restrict__ gmargin, uint32_t* __restrict__ gdisp,
                                                 const CarryStore& cs, const int* __restrict__ rmap = nullptr, const int* __restrict__ gfull = nullptr,
                                                 const int32_t* __restrict__ part = nullptr, const uint8_t* __restrict__ line_tab = nullptr)
{
	auto sym_of = [&](int f) -> const uint8_t* {
		if constexpr (RESCUE) return f < 0 ? cs.symbols + (size_t)~f * CS_CELLS : symbols + (size_t)f * NCELLS;
		else if constexpr (CARRY) return f < CARRY_SLOTS ? cs.symbols + (size_t)f * CS_CELLS : symbols + (size_t)(f - CARRY_SLOTS) * NCELLS;
		else return symbols + (size_t)f * NCELLS;
	};
	auto col_of = [&](int f) -> const uint8_t* {
		if constexpr (RESCUE) return f < 0 ? cs.colors + (size_t)~f * CS_CELLS : colors + (size_t)f * NCELLS;
		else if constexpr (CARRY) return f < CARRY_SLOTS ? cs.colors + (size_t)f * CS_CELLS : colors + (size_t)(f - CARRY_SLOTS) * NCELLS;
		else return colors + (size_t)f * NCELLS;
	};
	auto drift_of = [&](int f) -> const int8_t* {
		if constexpr (RESCUE) return f < 0 ? cs.drift + (size_t)~f * CS_DRIFT : drift + (size_t)f * NCELLS * 2;
		else if constexpr (CARRY) return f < CARRY_SLOTS ? cs.drift + (size_t)f * CS_DRIFT : drift + (size_t)(f - CARRY_SLOTS) * NCELLS * 2;
		else return drift + (size_t)f * NCELLS * 2;
	};
	auto plane_of = [&](int f) -> const uint32_t* {
		if constexpr (RESCUE) return f < 0 ? cs.plane + (size_t)~f * CS_PLANE : plane + (size_t)f * PLANE_WORDS;
		else if constexpr (CARRY) return f < CARRY_SLOTS ? cs.plane + (size_t)f * CS_PLANE : plane + (size_t)(f - CARRY_SLOTS) * PLANE_WORDS;
		else return plane + (size_t)f * PLANE_WORDS;
	};
	auto flood_of = [&](int f) -> uint32_t {
		if constexpr (RESCUE) return f < 0 ? cs.flood[~f] : flood_flag[f];
		else if constexpr (CARRY) return f < CARRY_SLOTS ? cs.flood[f] : flood_flag[f - CARRY_SLOTS];
		else return flood_flag[f];
	};
	const int g = blockIdx.y;
	if (g >= *ngroups) return;
	__shared__ int s_mem[GMAX];
	__shared__ uint32_t s_flood[GMAX];
	__shared__ uint16_t s_q[4][GC_CELLS / 4];
	const int m = gcount[g];
	if (threadIdx.x < GMAX) {
		int f = (int)threadIdx.x < m ? gmem[(size_t)g * GMAX + threadIdx.x] : 0;
		if constexpr (RESCUE) f = (int)threadIdx.x < m ? rmap[f] : 0;
		s_mem[threadIdx.x] = f;
		s_flood[threadIdx.x] = (int)threadIdx.x < m ? flood_of(f) : 0u;
	}
	// (SALVAGE: the members' line ranges, in LDS only. Members 0 .. gfull[g] - 1 are full; the partials behind them come from the slot's row
	// of `part`, the preceding one first where the group took it)
	__shared__ uint8_t s_rng[SALVAGE ? GMAX : 1][4];                     // {axis, lo, hi, 0}
	if constexpr (SALVAGE) {
		if (threadIdx.x < GMAX) {
			const int c = (int)threadIdx.x - gfull[g];
			const int32_t* row = part + (size_t)g * 8;
			const int32_t* p = (c == 0 && row[0] >= 0) ? row : row + 4;
			const bool full = c < 0 || (int)threadIdx.x >= m;
			s_rng[threadIdx.x][0] = full ? 0 : (uint8_t)p[1];
			s_rng[threadIdx.x][1] = full ? 0 : (uint8_t)p[2];
			s_rng[threadIdx.x][2] = full ? 255 : (uint8_t)p[3];
		}
	}
	// member c takes part in cell i (bit c of `who`, SALVAGE only)
	auto who_of = [&](int i) -> uint32_t {
		uint32_t who = 0;
		if constexpr (SALVAGE) {
			const uint32_t ln[2] = {line_tab[i], line_tab[NCELLS + i]};
#pragma unroll
			for (int c = 0; c < GMAX; ++c) {
				const uint32_t l = ln[s_rng[c][0] & 1];
				who |= (c < m && s_rng[c][1] <= l && l < s_rng[c][2]) ? 1u << c : 0u;
			}
		}
		return who;
	};
	__syncthreads();
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	uint8_t* os = gsym + (size_t)g * NCELLS;
	uint8_t* oc = gcol + (size_t)g * NCELLS;
	uint16_t* om = gmargin + (size_t)g * NCELLS;
	// phase 1
	int qn = 0;
	bool differ = false;
#pragma unroll
	for (int r = 0; r < GC_CELLS / 256; ++r) {
		const int i = blockIdx.x * GC_CELLS + r * 256 + (int)threadIdx.x;
		bool need = false;
		if (i < NCELLS) {
			uint32_t sy[GMAX], co[GMAX];
			bool sym_eq = true;
			const uint32_t who = who_of(i);
			auto in = [&](int c) -> bool {
				if constexpr (SALVAGE) return ((who >> c) & 1u) != 0;
				else return c < m;
			};
			const int np = SALVAGE ? (int)__popc(who) : m;                  // the cell's participants
#pragma unroll
			for (int c = 0; c < GMAX; ++c) {
				sy[c] = in(c) ? sym_of(s_mem[c])[i] & 15u : 0u;
				co[c] = in(c) ? col_of(s_mem[c])[i] : 0u;
				sym_eq = sym_eq && (!in(c) || sy[c] == sy[0]);
			}
			// plurality: the first member's colour among those with the most votes, and whether another colour has as many
			int best = 0;
			uint32_t win = co[0];
			bool tie = false;
#pragma unroll
			for (int c = 0; c < GMAX; ++c) {
				int v = 0;
#pragma unroll
				for (int q = 0; q < GMAX; ++q) v += (in(c) && in(q) && co[q] == co[c]) ? 1 : 0;
				if (in(c)) {
					if (v > best) { best = v; win = co[c]; tie = false; }
					else if (v == best && co[c] != win) tie = true;
				}
			}
			need = np > 1 && (!sym_eq || tie);
			differ = differ || !sym_eq || best != np;
			if (!need) {
				os[i] = (uint8_t)sy[0];
				oc[i] = (uint8_t)win;
				om[i] = MARGIN_NONE;
			}
		}
		const unsigned long long qb = __ballot(need);
		if (need) s_q[wv][qn + (int)__popcll(qb & ((1ull << lane) - 1ull))] = (uint16_t)i;
		qn += (int)__popcll(qb);
	}
	if (__ballot(differ) && lane == 0) gdisp[g] = 1u;   // (zeroed by the host; every writer writes 1)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// phase 2: one disputed cell per lane
	for (int q = lane; q < qn; q += 64) {
		const int i = s_q[wv][q];
		const ushort2 xy = tb.cell_xy[i];
		uint64_t H[GMAX];
		uint32_t sy[GMAX], co[GMAX];
		int score[16];
#pragma unroll
		for (int t = 0; t < 16; ++t) score[t] = 0;
		bool sym_eq = true;
		const uint32_t who = who_of(i);
		auto in = [&](int c) -> bool {
			if constexpr (SALVAGE) return ((who >> c) & 1u) != 0;
			else return c < m;
		};
#pragma unroll
		for (int c = 0; c < GMAX; ++c) {
			H[c] = 0;
			sy[c] = co[c] = 0;
			if (in(c)) {
				const int f = s_mem[c];
				sy[c] = sym_of(f)[i] & 15u;
				co[c] = col_of(f)[i];
				const bool flooded = s_flood[c] != 0;
				const int8_t* dr = drift_of(f);
				const int dx = flooded ? dr[(size_t)i * 2] : 0, dy = flooded ? dr[(size_t)i * 2 + 1] : 0;
				uint32_t rows[10];
				window_rows(plane_of(f), (int)xy.x + dx - 1, (int)xy.y + dy - 1, rows);
				H[c] = window_hash(rows, 4);
#pragma unroll
				for (int t = 0; t < 16; ++t) score[t] += 2 * (int)__popcll(H[c] ^ c_tile[t]) - (sy[c] == (uint32_t)t ? 1 : 0);
				sym_eq = sym_eq && sy[c] == sy[0];
			}
		}
		uint32_t s_hat = sy[0];
		uint16_t margin = MARGIN_NONE;
		if (!sym_eq) {
			int lo = score[0], second = 0x7FFFFFFF;
			s_hat = 0;
#pragma unroll
			for (int t = 1; t < 16; ++t) {
				if (score[t] < lo) { second = lo; lo = score[t]; s_hat = (uint32_t)t; }
				else if (score[t] < second) second = score[t];
			}
			margin = (uint16_t)(second - lo);
		}
		int best = 0, bd = 0x7FFFFFFF;
		uint32_t win = co[0];
		bool tie = false;
		int votes[GMAX];
#pragma unroll
		for (int c = 0; c < GMAX; ++c) {
			int v = 0;
#pragma unroll
			for (int q2 = 0; q2 < GMAX; ++q2) v += (in(c) && in(q2) && co[q2] == co[c]) ? 1 : 0;
			votes[c] = v;
			if (in(c)) {
				if (v > best) { best = v; win = co[c]; tie = false; }
				else if (v == best && co[c] != win) tie = true;
			}
		}
		if (tie) {
#pragma unroll
			for (int c = 0; c < GMAX; ++c) {
				const int d = (int)__popcll(H[c] ^ c_tile[s_hat]);
				if (in(c) && votes[c] == best && d < bd) { bd = d; win = co[c]; }
			}
		}
		os[i] = (uint8_t)s_hat;
		oc[i] = (uint8_t)win;
		om[i] = margin;
	}
}


__global__ __launch_bounds__(256) void k_group_cells(const uint32_t* __restrict__ plane, Tables tb, const uint8_t* __restrict__ symbols,
                                                     const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                     const uint32_t* __restrict__ flood_flag, const int* __restrict__ gmem,
                                                     const int* __restrict__ gcount, const int* __restrict__ ngroups, uint8_t* __restrict__ gsym,
                                                     uint8_t* __restrict__ gcol, uint16_t* __restrict__ gmargin, uint32_t* __restrict__ gdisp)
{
	group_cells_body<false>(plane, tb, symbols, colors, drift, flood_flag, gmem, gcount, ngroups, gsym, gcol, gmargin, gdisp, CarryStore{});
}

// G4: one workgroup per group slot (n of them). A slot at or above the group count, or a group left without members, gets zero chunks and
// mask 0. Otherwise:
//   cmask  the aligned_stream bookkeeping over the combined decode's block flags, the symbol blocks then the colour blocks with one state
//          (what k_frame_mid and k_frame_end do for one frame; legacy modes: the one coupled stream)
//   chunk j of the group = the combined decode's chunk j where cmask has it, else member chunk j of the lowest-index member that delivered it
//   e_on   (erasure decoding, modes 68 / 67 / 66): every block of a symbol chunk still missing is decoded again (er_retry_blocks) -- a block
//          errors-only decoding accepted with no erasures, a failed block with the stream bytes of the symbol-disputed cells as erasures
//          (smallest margin first, then stream position, at most e_max). A chunk whose blocks are all accepted joins the mask with its bytes.
// gmask = cmask | the members' masks | the chunks the retry added; slots of chunks outside it are zero.
// (CARRY: a member id is a carry slot or CARRY_SLOTS + a batch index, as in G3, and the member count of every slot goes to gsizes)
template <bool CARRY>
__device__ __forceinline__ void group_end_body(const uint8_t* __restrict__ gsym, const uint16_t* __restrict__ gmargin, const Tables& tb,
                                               const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                               const uint8_t* __restrict__ grs_ok, const uint8_t* __restrict__ chunks,
                                               const uint32_t* __restrict__ masks, const uint32_t* __restrict__ gdisp, uint8_t* __restrict__ gchunks,
                                               uint32_t* __restrict__ gmasks, int e_on, int e_max, const CarryStore& cs, int* __restrict__ gsizes)
{
	const int g = blockIdx.x;
	uint8_t* gc = gchunks + (size_t)g * FRAME_BYTES;
	const int m = g < *ngroups ? gcount[g] : 0;
	if constexpr (CARRY) { if (threadIdx.x == 0) gsizes[g] = m; }
	if (m == 0) {
		for (int k = threadIdx.x; k < FRAME_BYTES; k += 256) gc[k] = 0;
		if (threadIdx.x == 0) gmasks[g] = 0;
		return;
	}
	constexpr uint32_t FULL = (1u << CHUNKS) - 1u, SYM_MASK = LEGACY ? 0u : (1u << SYM_CHUNKS) - 1u;
	__shared__ int s_mem[GMAX];
	__shared__ uint32_t s_mmask[GMAX];
	__shared__ uint32_t s_cmask;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	if (threadIdx.x < GMAX) {
		const int f = (int)threadIdx.x < m ? gmem[(size_t)g * GMAX + threadIdx.x] : 0;
		s_mem[threadIdx.x] = f;
		if constexpr (CARRY) s_mmask[threadIdx.x] = (int)threadIdx.x < m ? (f < CARRY_SLOTS ? cs.masks[f] : masks[f - CARRY_SLOTS]) : 0u;
		else s_mmask[threadIdx.x] = (int)threadIdx.x < m ? masks[f] : 0u;
	}
	// a group whose members agree on every cell has each member's cells, so its combined decode is each member's errors-only decode (a
	// subset of the member's mask, the same bytes) and the retry finds no disputed cell: the members' chunks are the whole answer, and the
	// Reed-Solomon pass skipped it (k_rs LIVE)
	const bool disp = gdisp[g] != 0;
	if (threadIdx.x == 0) s_cmask = 0;
	if (wv == 0 && disp) {
		const uint8_t* ok = grs_ok + (size_t)g * ALL_BLOCKS;
		static_assert(ALL_BLOCKS <= 128, "block flags fit two ballots");
		const unsigned long long lo = __ballot(lane < ALL_BLOCKS && ok[lane < ALL_BLOCKS ? lane : 0] != 0);
		const unsigned long long hi = ALL_BLOCKS > 64 ? __ballot(64 + lane < ALL_BLOCKS && ok[64 + lane < ALL_BLOCKS ? 64 + lane : 0] != 0) : 0ull;
		if (lane == 0) {
			FrameState st = {0, 0, 0, 0};
			uint8_t hdr[6] = {0, 0, 0, 0, 0, 0};
			unsigned radio = 0;
			for (int b = 0; b < ALL_BLOCKS; ++b) aligner_block(st, b, (int)(((b < 64 ? lo : hi) >> (b & 63)) & 1ull), nullptr, false, hdr, radio);
			s_cmask = st.mask;
		}
	}
	__syncthreads();
	const uint32_t cmask = s_cmask;
	uint32_t mmask = 0;
	for (int c = 0; c < m; ++c) mmask |= s_mmask[c];
	uint32_t emask = 0;
	if constexpr (!LEGACY) {
		const uint32_t missing = SYM_MASK & ~(cmask | mmask);
		if (e_on && disp && missing) {
			const uint8_t* sym = gsym + (size_t)g * NCELLS;
			const uint16_t* mg = gmargin + (size_t)g * NCELLS;
			emask = er_retry_blocks<uint16_t, 0, SYM_BLOCKS>(missing, grs_ok + (size_t)g * ALL_BLOCKS, e_max, gc, [&](int b, int k, bool) {
				const int sidx = (RS_BLOCK * b + k) * 2;
				const int c0 = tb.stream_cell[sidx], c1 = tb.stream_cell[sidx + 1];
				const uint32_t m0 = mg[c0], m1 = mg[c1];
				// smallest margin first is highest score first with score = 0xFFFF - margin, ties to the lower byte either way, and an
				// undisputed byte (both MARGIN_NONE = 0xFFFF) scores 0: not flagged. The score still fits the 16 bits of the margin.
				return ErByte{((sym[c0] & 15u) << 4) | (sym[c1] & 15u), (int)(0xFFFFu - (m0 < m1 ? m0 : m1))};
			});
		}
	}
	for (int j = 0; j < CHUNKS; ++j) {
		const uint32_t bit = 1u << j;
		if (cmask & bit) continue;
		uint8_t* dst = gc + (size_t)j * CHUNK;
		if (mmask & bit) {
			int c = 0;
			while (!(s_mmask[c] & bit)) ++c;
			const uint8_t* src;
			if constexpr (CARRY) src = (s_mem[c] < CARRY_SLOTS ? cs.chunks + (size_t)s_mem[c] * CS_CHUNKS : chunks + (size_t)(s_mem[c] - CARRY_SLOTS) * FRAME_BYTES) + (size_t)j * CHUNK;
			else src = chunks + (size_t)s_mem[c] * FRAME_BYTES + (size_t)j * CHUNK;
			for (int k = threadIdx.x; k < CHUNK; k += 256) dst[k] = src[k];
		} else if (!(emask & bit)) {
			for (int k = threadIdx.x; k < CHUNK; k += 256) dst[k] = 0;
		}
	}
	if (threadIdx.x == 0) gmasks[g] = (cmask | mmask | emask) & FULL;
}

__global__ __launch_bounds__(256) void k_group_end(const uint8_t* __restrict__ gsym, const uint16_t* __restrict__ gmargin, Tables tb,
                                                   const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                                   const uint8_t* __restrict__ grs_ok, const uint8_t* __restrict__ chunks,
                                                   const uint32_t* __restrict__ masks, const uint32_t* __restrict__ gdisp, uint8_t* __restrict__ gchunks,
                                                   uint32_t* __restrict__ gmasks, int e_on, int e_max)
{
	group_end_body<false>(gsym, gmargin, tb, gmem, gcount, ngroups, grs_ok, chunks, masks, gdisp, gchunks, gmasks, e_on, e_max, CarryStore{}, nullptr);
}

// ------------------------------------------------------------------------------------------------ colour vote and group colour retry
// Opt-in (modes 68 / 67 / 66): cimbar_hip_set_group_colour_vote for the plain combined calls, cimbar_hip_set_stream_colour_vote for the stream calls
// (k_group_colour_stream and k_group_carry_weights under "the stream calls"). With a call's setting off none of these kernels is launched.
// G3c k_group_colour, behind G3 and in front of the groups' Reed-Solomon pass: one workgroup per group slot; a slot at or above the group count
// and a group G3 did not flag (gdisp: no cell differs) return at once. For a cell whose members' colours differ (a "colour dispute"):
//   w_c      = margin_c + 1, margin_c = color_fit<true> of member c from exactly what k_colors classified the cell from -- the K1 cell mean, or
//              mean6x6 at the drifted position where the member took the flood pass -- under the member's matrix in force (ccm_used, active flag
//              included): what CIMBAR_HIP_TAP_COLOUR_MARGIN defines. The + 1 lets a zero-margin member still decide between colours nobody
//              else voted for.
//   score(k) = sum of w_c over the members with col_c == k (u32: at most 8 * 390 151)
//   colour   = argmax score, ties to the lowest colour index; gm = the best score minus the second-best (a colour nobody voted for scores 0)
// gcol gets the colour, gcm the margin gm, gcw[member capture] the weight. A cell without a colour dispute keeps G3's colour, gcm = GCM_NONE
// and weight 0. The symbol side (gsym, gmargin) is not touched. Nothing is written for an unflagged group: the taps fill those in.
// Phase 1 compares the members' colour bytes four cells per dword, settles the agreeing cells (16-byte stores where all four agree) and queues
// the disputed ones per wavefront; phase 2 gives each queued cell a lane. The scores live in NCOLORS registers; the member loop is not unrolled.
constexpr uint32_t GCM_NONE = 0xFFFFFFFFu;
constexpr int GV_WORDS = NCELLS / 4, GV_ROUNDS = (GV_WORDS + 255) / 256, GV_QCAP = GV_ROUNDS * 64 * 4;   // a wavefront's share of the cells at most
static_assert(NCELLS <= 65536, "a queued cell index fits 16 bits");

// (CARRY = false is the plain calls' kernel as it always was. CARRY, the stream calls' k_group_colour_stream: a member id below CARRY_SLOTS names a
// carry slot, as in G3 -- its colour byte comes from cs.colors and its weight from the row k_group_carry_weights wrote while the member's batch was
// on the device, so neither a mean nor a matrix is read for it, and it has no gcw row: gcw has one row per capture of the call)
template <bool CARRY>
__device__ __forceinline__ void group_colour_body(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, const Tables& tb,
                                                  const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                  const uint32_t* __restrict__ flood_flag, const float* __restrict__ ccm_used,
                                                  const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                                  const uint32_t* __restrict__ gdisp, uint8_t* __restrict__ gcol, uint32_t* __restrict__ gcm,
                                                  uint32_t* __restrict__ gcw, const CarryStore& cs)
{
	if constexpr (LEGACY) return;                          // (one coupled stream: the host never launches it there)
	// a member id -> is it a carry slot, its index in the call's batch, its colour bytes
	auto carried = [&](int f) -> bool {
		if constexpr (CARRY) return f < CARRY_SLOTS;
		else return false;
	};
	auto cap_of = [&](int f) -> int {
		if constexpr (CARRY) return f - CARRY_SLOTS;
		else return f;
	};
	auto col_of = [&](int f) -> const uint8_t* {
		if constexpr (CARRY) return f < CARRY_SLOTS ? cs.colors + (size_t)f * CS_CELLS : colors + (size_t)(f - CARRY_SLOTS) * NCELLS;
		else return colors + (size_t)f * NCELLS;
	};
	const int g = blockIdx.x;
	if (g >= *ngroups || gdisp[g] == 0) return;            // (uniform over the workgroup)
	const int m = gcount[g] < GMAX ? gcount[g] : GMAX;
	__shared__ int s_mem[GMAX];
	__shared__ uint32_t s_flood[GMAX];
	__shared__ float s_ccm[GMAX][10];
	__shared__ uint16_t s_q[4][GV_QCAP];
	if (threadIdx.x < GMAX) {
		const int f = (int)threadIdx.x < m ? gmem[(size_t)g * GMAX + threadIdx.x] : 0;
		s_mem[threadIdx.x] = f;
		s_flood[threadIdx.x] = ((int)threadIdx.x < m && !carried(f)) ? flood_flag[cap_of(f)] : 0u;
	}
	if (threadIdx.x < GMAX * 10) {
		const int c = threadIdx.x / 10, k = threadIdx.x % 10;
		const int f = c < m ? gmem[(size_t)g * GMAX + c] : 0;
		s_ccm[c][k] = (c < m && !carried(f)) ? ccm_used[(size_t)cap_of(f) * 10 + k] : 0.0f;
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	uint8_t* oc = gcol + (size_t)g * NCELLS;
	uint32_t* om = gcm + (size_t)g * NCELLS;
	constexpr uint32_t CM = 0x01010101u * (uint32_t)(NCOLORS - 1);
	// phase 1
	int qn = 0;
	for (int r = 0; r < GV_ROUNDS; ++r) {
		const int w = r * 256 + (int)threadIdx.x;
		uint32_t x = 0;
		if (w < GV_WORDS) {
			const uint32_t c0 = reinterpret_cast<const uint32_t*>(col_of(s_mem[0]))[w];
			for (int c = 1; c < m; ++c) x |= (reinterpret_cast<const uint32_t*>(col_of(s_mem[c]))[w] ^ c0) & CM;
			if (x == 0) {
				reinterpret_cast<uint4*>(om)[w] = make_uint4(GCM_NONE, GCM_NONE, GCM_NONE, GCM_NONE);
				for (int c = 0; c < m; ++c)
					if (!carried(s_mem[c])) reinterpret_cast<uint4*>(gcw + (size_t)cap_of(s_mem[c]) * NCELLS)[w] = make_uint4(0u, 0u, 0u, 0u);
			} else {
#pragma unroll
				for (int b = 0; b < 4; ++b)
					if (((x >> (8 * b)) & 0xFFu) == 0) {
						om[4 * w + b] = GCM_NONE;
						for (int c = 0; c < m; ++c)
							if (!carried(s_mem[c])) gcw[(size_t)cap_of(s_mem[c]) * NCELLS + 4 * w + b] = 0u;
					}
			}
		}
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const bool need = ((x >> (8 * b)) & 0xFFu) != 0;
			const unsigned long long qb = __ballot(need);
			if (need) s_q[wv][qn + (int)__popcll(qb & ((1ull << lane) - 1ull))] = (uint16_t)(4 * w + b);
			qn += (int)__popcll(qb);
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// phase 2: one colour-disputed cell per lane
	for (int q = lane; q < qn; q += 64) {
		const int i = s_q[wv][q];
		const ushort2 xy = tb.cell_xy[i];
		const uint32_t slot = tb.cell_grid[i];
		uint32_t score[NCOLORS];
#pragma unroll
		for (int k = 0; k < NCOLORS; ++k) score[k] = 0;
		for (int c = 0; c < m; ++c) {
			if constexpr (CARRY) {
				if (carried(s_mem[c])) {               // its weight was taken when its batch was on the device; no gcw row
					const uint32_t wgt = cs.weights[(size_t)s_mem[c] * CS_WEIGHTS + i];
					const uint32_t mine = col_of(s_mem[c])[i] & (uint32_t)(NCOLORS - 1);
#pragma unroll
					for (int k = 0; k < NCOLORS; ++k) score[k] += mine == (uint32_t)k ? wgt : 0u;
					continue;
				}
			}
			const int f = cap_of(s_mem[c]);
			uint32_t col[3];
			if (s_flood[c] != 0) {
				const int x = (int)xy.x + drift[((size_t)f * NCELLS + i) * 2], y = (int)xy.y + drift[((size_t)f * NCELLS + i) * 2 + 1];
				mean6x6(rgb + (size_t)f * FRAME_RGB, x + 1, y + 1, col);
			} else {
				const uint32_t mv = cellmean[(size_t)f * GRID_CELLS + slot];
				col[0] = mv & 0xFFu; col[1] = (mv >> 8) & 0xFFu; col[2] = (mv >> 16) & 0xFFu;
			}
			const uint32_t wgt = color_fit<true>((float)col[0], (float)col[1], (float)col[2], s_ccm[c], s_ccm[c][9] != 0.0f).margin + 1u;
			const uint32_t mine = colors[(size_t)f * NCELLS + i] & (uint32_t)(NCOLORS - 1);
#pragma unroll
			for (int k = 0; k < NCOLORS; ++k) score[k] += mine == (uint32_t)k ? wgt : 0u;
			gcw[(size_t)f * NCELLS + i] = wgt;
		}
		uint32_t best = score[0], second = 0, win = 0;
#pragma unroll
		for (int k = 1; k < NCOLORS; ++k) {
			if (score[k] > best) { second = best; best = score[k]; win = (uint32_t)k; }
			else if (score[k] > second) second = score[k];
		}
		oc[i] = (uint8_t)win;
		om[i] = best - second;
	}
}

__global__ __launch_bounds__(256) void k_group_colour(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                      const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                      const uint32_t* __restrict__ flood_flag, const float* __restrict__ ccm_used,
                                                      const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                                      const uint32_t* __restrict__ gdisp, uint8_t* __restrict__ gcol, uint32_t* __restrict__ gcm,
                                                      uint32_t* __restrict__ gcw)
{
	group_colour_body<false>(rgb, cellmean, tb, colors, drift, flood_flag, ccm_used, gmem, gcount, ngroups, gdisp, gcol, gcm, gcw, CarryStore{});
}

// G4c k_group_colour_retry, behind G4 (armed by the vote together with cimbar_hip_set_colour_erasure_decode): k_colour_erasure_frame's retry over
// the group's cells, a kernel of its own so that the frame retry's code stays what it was. One workgroup per group slot; a slot at or above
// the count, a group without members, an unflagged group (nothing disputed: nothing to flag, and its Reed-Solomon pass was skipped) and a
// group whose colour chunks are all in gmask return at once. Otherwise, for the colour chunks gmask lacks after G4's fill:
//  * a colour-stream byte's score is max over its four cells of c_margin - gm; a cell without a colour dispute contributes nothing; flagged
//    when > 0
//  * retry, acceptance and the mask update are er_retry_blocks and er_commit over the colour blocks; chunks already in gmask are never
//    rewritten, the slots of colour chunks still missing are zeroed again
__global__ __launch_bounds__(256) void k_group_colour_retry(const uint8_t* __restrict__ gcol, const uint32_t* __restrict__ gcm, Tables tb,
                                                            const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                                            const uint32_t* __restrict__ gdisp, const uint8_t* __restrict__ grs_ok,
                                                            uint8_t* __restrict__ gchunks, uint32_t* __restrict__ gmasks, int c_margin, int e_max)
{
	if constexpr (LEGACY) return;
	constexpr uint32_t COL_MASK = ((1u << COL_CHUNKS) - 1u) << SYM_CHUNKS;
	const int g = blockIdx.x;
	if (g >= *ngroups || gcount[g] == 0 || gdisp[g] == 0) return;   // (uniform over the workgroup)
	const uint32_t mask = gmasks[g];
	if ((mask & COL_MASK) == COL_MASK) return;
	const uint8_t* cf = gcol + (size_t)g * NCELLS;
	const uint32_t* mg = gcm + (size_t)g * NCELLS;
	uint8_t* fc = gchunks + (size_t)g * FRAME_BYTES;
	const uint32_t done = er_retry_blocks<int32_t, SYM_BLOCKS, COL_BLOCKS>(COL_MASK & ~mask, grs_ok + (size_t)g * ALL_BLOCKS, e_max, fc, [&](int b, int k, bool ok) {
		const int sidx = (RS_BLOCK * (b - SYM_BLOCKS) + k) * 4;
		int best = INT_MIN;
		uint32_t v = 0;
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const int cell = tb.stream_cell[sidx + q];
			v = (v << 2) | (cf[cell] & 3u);
			if (!ok) {
				const uint32_t gm = mg[cell];
				const int sc = gm == GCM_NONE ? INT_MIN : c_margin - (int)gm;
				best = sc > best ? sc : best;
			}
		}
		return ErByte{v, best};
	});
	er_commit(mask | done, gmasks + g, fc, SYM_CHUNKS, CHUNKS);
}

// ------------------------------------------------------------------------------------------------ the stream calls
// cimbar_hip_decode_batch_combined_stream / _scan_extract_decode_batch_combined_stream_fmt: the same decode over a VIRTUAL batch, the c = *cs.count
// carried members (one group by construction, c < max_group) followed by the call's n captures. Virtual capture j < c is carry slot j, virtual
// capture j >= c is capture k = j - c of the call. Only groups that CLOSE in the call get ids, are decoded (G3, k_rs LIVE, G4 run over
// n + 1 group slots) and reported; the group still open at the end is copied into the carry store by k_group_carry. c, the open group and
// its members never leave the device.
// With cimbar_hip_set_stream_colour_vote on, the colour vote runs over the virtual batch as well (G3cs k_group_colour_stream, G4c as it is): the
// carry store then holds the vote's weight of every cell of every carried member (G5w k_group_carry_weights) -- weights, not means or matrices.

// G1s: one workgroup per capture k < n: agree[k] = agree(predecessor, k), the predecessor being capture k - 1 or, for k = 0, the last
// carried member (nothing carried: agree[0] is not written and not read)
__global__ __launch_bounds__(256) void k_group_agree_stream(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n, CarryStore cs,
                                                            uint32_t* __restrict__ agree)
{
	const int k = blockIdx.x;
	if (k >= n) return;
	const int c = *cs.count;
	if (k == 0 && c == 0) return;
	const uint32_t* s1 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
	const uint32_t* c1 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
	const uint32_t* s0 = k > 0 ? s1 - NCELLS / 4 : reinterpret_cast<const uint32_t*>(cs.symbols + (size_t)(c - 1) * CS_CELLS);
	const uint32_t* c0 = k > 0 ? c1 - NCELLS / 4 : reinterpret_cast<const uint32_t*>(cs.colors + (size_t)(c - 1) * CS_CELLS);
	const uint32_t a = agreeing_cells(s0, c0, s1, c1);
	if (threadIdx.x == 0) agree[k] = a;
}

// G2s: k_group_walk's walk (groups_in == nullptr) over the virtual batch, 64 virtual captures per step. Virtual capture j starts a group when it is
// usable and j == 0, or j - 1 is unusable, or j >= max(c, 1) and agree[j - c] * 1000 < min_agree * NCELLS, or the group before already has max_group
// members -- so the carried members open group 0 and count toward its cap. The LAST group stays open when there is no flush, its last member
// is the last virtual capture (which is then usable) and it has fewer than max_group members; every other group closes.
//   groups[k]   the id of capture k's group or -1 (the open group's members get its id here; k_group_carry turns them into GROUP_OPEN)
//   gmem/gcount as in k_group_walk, a member being its carry slot (j < c) or CARRY_SLOTS + k; n + 1 group slots, gcount zeroed by the host
//   *ngroups    the groups that close in this call (the open one has the id *ngroups); *open_size = the open group's members or 0
// What a step hands to the next is either a ballot's popcount or a __shfl of lane 63, read back through readfirstlane so that it stays in
// scalar registers whatever the compiler can prove.
__global__ __launch_bounds__(64) void k_group_walk_stream(const uint32_t* __restrict__ agree, int n, const int* __restrict__ status, int stride,
                                                          int min_agree, int max_group, int flush, CarryStore cs, int* __restrict__ groups,
                                                          int* __restrict__ gmem, int* __restrict__ gcount, int* __restrict__ ngroups,
                                                          int* __restrict__ open_size)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
	const int c = __builtin_amdgcn_readfirstlane(*cs.count);
	const int N = c + n;
	int run_carry = 0, starts_carry = 0, mem_carry = 0, base_carry = 0, prev_id = -1, top = -1;
	bool prev_u = false, last_u = false;
	auto fetch = [&](int j, uint32_t& a, int& st) {
		const int k = j - c;
		a = (j > 0 && k >= 0 && j < N) ? agree[k] : 0xFFFFFFFFu;      // (inside the carried group: agreement is implied)
		st = (status && k >= 0 && j < N) ? status[(size_t)k * stride] : 1;
	};
	uint32_t a_cur; int st_cur;
	fetch(lane, a_cur, st_cur);
	for (int j0 = 0; j0 < N; j0 += 64) {
		const int j = j0 + lane;
		uint32_t a_nxt; int st_nxt;
		fetch(j + 64, a_nxt, st_nxt);
		const bool in = j < N;
		const bool u = in && st_cur > 0;
		const unsigned long long ub = __ballot(u);
		if (N - 1 - j0 < 64) last_u = ((ub >> (N - 1 - j0)) & 1ull) != 0;
		const bool u_prev = lane == 0 ? prev_u : ((ub >> (lane - 1)) & 1ull) != 0;
		const bool brk = in && (j == 0 || !u_prev || (j >= c && (unsigned long long)a_cur * 1000ull < (unsigned long long)min_agree * NCELLS));
		const unsigned long long bb = __ballot(brk) & upto;
		const int run = bb ? j0 + 63 - __clzll(bb) : run_carry;          // the latest break at or before j
		const bool start = u && (j - run) % max_group == 0;
		const unsigned long long sb = __ballot(start);
		const int id = u ? starts_carry + (int)__popcll(sb & upto) - 1 : -1;
		run_carry = __builtin_amdgcn_readfirstlane(__shfl(run, 63));
		starts_carry += (int)__popcll(sb);
		const int id_prev_lane = __shfl(id, lane > 0 ? lane - 1 : 0);
		const int id_prev = lane == 0 ? prev_id : id_prev_lane;
		const bool head = id >= 0 && (j == 0 || id_prev != id);
		const bool member = id >= 0;
		const unsigned long long mb = __ballot(member), hb = __ballot(head) & upto;
		const int before = mem_carry + (int)__popcll(mb & below);           // members of the virtual batch in front of j
		const int hl = hb ? 63 - __clzll(hb) : lane;
		const int at_head = __shfl(before, hl);
		const int base = hb ? at_head : base_carry;                          // members in front of j's group
		if (in && j >= c) groups[j - c] = id;
		if (member) {
			gmem[(size_t)id * GMAX + (before - base)] = j < c ? j : CARRY_SLOTS + (j - c);
			atomicAdd(&gcount[id], 1);
		}
		top = id > top ? id : top;
		prev_id = __builtin_amdgcn_readfirstlane(__shfl(id, 63));
		prev_u = __builtin_amdgcn_readfirstlane(__shfl((int)u, 63)) != 0;
		mem_carry += (int)__popcll(mb);
		base_carry = __builtin_amdgcn_readfirstlane(__shfl(base, 63));
		a_cur = a_nxt; st_cur = st_nxt;
	}
	for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(top, o); top = t > top ? t : top; }
	// lanes past the last virtual capture are in no group and head none, so lane 63's base is the last group's: its size is what follows it
	const int last_size = top >= 0 ? mem_carry - base_carry : 0;
	const bool open = !flush && top >= 0 && last_u && last_size < max_group;
	if (lane == 0) {
		*ngroups = open ? top : top + 1;
		*open_size = open ? last_size : 0;
	}
}

__global__ __launch_bounds__(256) void k_group_cells_stream(const uint32_t* __restrict__ plane, Tables tb, const uint8_t* __restrict__ symbols,
                                                            const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                            const uint32_t* __restrict__ flood_flag, const int* __restrict__ gmem,
                                                            const int* __restrict__ gcount, const int* __restrict__ ngroups, uint8_t* __restrict__ gsym,
                                                            uint8_t* __restrict__ gcol, uint16_t* __restrict__ gmargin, uint32_t* __restrict__ gdisp,
                                                            CarryStore cs)
{
	group_cells_body<true>(plane, tb, symbols, colors, drift, flood_flag, gmem, gcount, ngroups, gsym, gcol, gmargin, gdisp, cs);
}

__global__ __launch_bounds__(256) void k_group_end_stream(const uint8_t* __restrict__ gsym, const uint16_t* __restrict__ gmargin, Tables tb,
                                                          const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ ngroups,
                                                          const uint8_t* __restrict__ grs_ok, const uint8_t* __restrict__ chunks,
                                                          const uint32_t* __restrict__ masks, const uint32_t* __restrict__ gdisp,
                                                          uint8_t* __restrict__ gchunks, uint32_t* __restrict__ gmasks, int e_on, int e_max, CarryStore cs,
                                                          int* __restrict__ gsizes)
{
	group_end_body<true>(gsym, gmargin, tb, gmem, gcount, ngroups, grs_ok, chunks, masks, gdisp, gchunks, gmasks, e_on, e_max, cs, gsizes);
}

// G3cs k_group_colour_stream (cimbar_hip_set_stream_colour_vote), behind G3s and in front of the groups' Reed-Solomon pass, n + 1 group slots: the
// colour vote over the virtual batch. The weight of a carried member is read from its carried row; everything else is k_group_colour.
__global__ __launch_bounds__(256) void k_group_colour_stream(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                             const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                             const uint32_t* __restrict__ flood_flag, const float* __restrict__ ccm_used,
                                                             const int* __restrict__ gmem, const int* __restrict__ gcount,
                                                             const int* __restrict__ ngroups, const uint32_t* __restrict__ gdisp,
                                                             uint8_t* __restrict__ gcol, uint32_t* __restrict__ gcm, uint32_t* __restrict__ gcw,
                                                             CarryStore cs)
{
	group_colour_body<true>(rgb, cellmean, tb, colors, drift, flood_flag, ccm_used, gmem, gcount, ngroups, gdisp, gcol, gcm, gcw, cs);
}

// bytes from src to dst by the whole workgroup: 16 bytes per lane where both ends and the length allow it, else dwords, else bytes
__device__ __forceinline__ void carry_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t bytes)
{
	const uintptr_t a = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
	if ((a & 15u) == 0) {
		const uint4* s = reinterpret_cast<const uint4*>(src);
		uint4* d = reinterpret_cast<uint4*>(dst);
		for (size_t k = threadIdx.x; k < bytes / 16; k += 256) d[k] = s[k];
	} else if ((a & 3u) == 0) {
		const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
		uint32_t* d = reinterpret_cast<uint32_t*>(dst);
		for (size_t k = threadIdx.x; k < bytes / 4; k += 256) d[k] = s[k];
	} else {
		for (size_t k = threadIdx.x; k < bytes; k += 256) dst[k] = src[k];
	}
}

// G5 k_group_carry, behind G4: the open group (*open_size members, gmem row *ngroups) becomes the carry store, member r in slot r; no open
// group: the store is empty. One workgroup per (slice, slot): CARRY_PARTS slices of each of the five arrays.
// A member that is itself carried needs no move and no staging copy: the carried members are the first virtual captures and open group 0,
// so in an open group that holds them member r IS slot r for every r < c, and only members from the call's batch (slots >= c, which no
// source occupies) are written. Slots at or above the new count keep stale bytes nothing reads.
// Workgroup (0, 0) also writes GROUP_OPEN over the open members' entries of groups[] and, last, the new count (every reader of the count
// is a later launch on the stream calls' order).
constexpr int CARRY_PARTS = 4, CARRY_ARRAYS = 5, GROUP_OPEN_ID = -2;
__global__ __launch_bounds__(256) void k_group_carry(const uint32_t* __restrict__ plane, const uint8_t* __restrict__ symbols,
                                                     const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                     const uint32_t* __restrict__ flood_flag, const uint8_t* __restrict__ chunks,
                                                     const uint32_t* __restrict__ masks, const int* __restrict__ gmem, const int* __restrict__ ngroups,
                                                     const int* __restrict__ open_size, int* __restrict__ groups, CarryStore cs)
{
	const int r = blockIdx.y, arr = blockIdx.x / CARRY_PARTS, part = blockIdx.x % CARRY_PARTS;
	const int m = *open_size;
	const int* mem = gmem + (size_t)*ngroups * GMAX;
	if (blockIdx.x == 0 && r == 0) {
		if ((int)threadIdx.x < m) { const int f = mem[threadIdx.x]; if (f >= CARRY_SLOTS) groups[f - CARRY_SLOTS] = GROUP_OPEN_ID; }
		if (threadIdx.x == 0) *cs.count = m;     // (read by this launch's other workgroups through open_size, never through the count)
	}
	if (r >= m) return;
	const int f = mem[r];
	if (f < CARRY_SLOTS) return;                 // already slot r
	const size_t k = (size_t)(f - CARRY_SLOTS);
	const uint8_t* src; uint8_t* dst; size_t bytes;
	switch (arr) {
		case 0: src = symbols + k * NCELLS; dst = cs.symbols + (size_t)r * CS_CELLS; bytes = NCELLS; break;
		case 1: src = colors + k * NCELLS; dst = cs.colors + (size_t)r * CS_CELLS; bytes = NCELLS; break;
		case 2: src = reinterpret_cast<const uint8_t*>(drift + k * NCELLS * 2); dst = reinterpret_cast<uint8_t*>(cs.drift + (size_t)r * CS_DRIFT); bytes = (size_t)NCELLS * 2; break;
		case 3: src = reinterpret_cast<const uint8_t*>(plane + k * PLANE_WORDS); dst = reinterpret_cast<uint8_t*>(cs.plane + (size_t)r * CS_PLANE); bytes = (size_t)PLANE_WORDS * 4; break;
		default: src = chunks + k * FRAME_BYTES; dst = cs.chunks + (size_t)r * CS_CHUNKS; bytes = FRAME_BYTES; break;
	}
	// this workgroup's slice: whole 16-byte units, the last slice takes the rest
	const size_t per = (bytes / CARRY_PARTS) & ~(size_t)15, lo = per * part, hi = part == CARRY_PARTS - 1 ? bytes : lo + per;
	carry_copy(dst + lo, src + lo, hi - lo);
	if (arr == 0 && part == 0 && threadIdx.x == 0) { cs.flood[r] = flood_flag[k]; cs.masks[r] = masks[k]; }
}

// G5w k_group_carry_weights (cimbar_hip_set_stream_colour_vote), next to G5 and behind every reader of the carried weights: the colour vote's
// weight of EVERY cell of the open group's members that come from the call's batch, w = color_fit<true>.margin + 1 from what k_colors classified
// the cell from under the member's matrix in force -- k_group_colour's weight, which depends on the member alone, evaluated while the member's
// means, frame and matrix are still on the device. One lane per cell, workgroup (cell block, slot r); r at or above the open group's size
// returns at once, and so does a member that is itself carried: it is slot r and keeps its row (k_group_carry's rule).
constexpr int CW_BLOCKS = (NCELLS + 255) / 256;
__global__ __launch_bounds__(256) void k_group_carry_weights(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                             const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                             const float* __restrict__ ccm_used, const int* __restrict__ gmem,
                                                             const int* __restrict__ ngroups, const int* __restrict__ open_size, CarryStore cs)
{
	if constexpr (LEGACY) return;                          // (the host never launches it there)
	const int r = blockIdx.y;
	if (r >= *open_size) return;                           // (uniform over the workgroup, as is the next)
	const int f = gmem[(size_t)*ngroups * GMAX + r];
	if (f < CARRY_SLOTS) return;                           // already slot r
	const size_t k = (size_t)(f - CARRY_SLOTS);
	__shared__ float s_m[10];
	if (threadIdx.x < 10) s_m[threadIdx.x] = ccm_used[k * 10 + threadIdx.x];
	__syncthreads();
	const int i = blockIdx.x * 256 + (int)threadIdx.x;
	if (i >= NCELLS) return;
	uint32_t col[3];
	if (flood_flag[k] != 0) {
		const ushort2 xy = tb.cell_xy[i];
		const int x = (int)xy.x + drift[(k * NCELLS + i) * 2], y = (int)xy.y + drift[(k * NCELLS + i) * 2 + 1];
		mean6x6(rgb + k * FRAME_RGB, x + 1, y + 1, col);
	} else {
		const uint32_t mv = cellmean[k * GRID_CELLS + tb.cell_grid[i]];
		col[0] = mv & 0xFFu; col[1] = (mv >> 8) & 0xFFu; col[2] = (mv >> 16) & 0xFFu;
	}
	cs.weights[(size_t)r * CS_WEIGHTS + i] = color_fit<true>((float)col[0], (float)col[1], (float)col[2], s_m, s_m[9] != 0.0f).margin + 1u;
}

// ------------------------------------------------------------------------------------------------ run rescue (the once-calls, opt-in)
// cimbar_hip_set_once_rescue: the group decode above over the runs of a plain once-call that stay incomplete after pass 2 (repeat.hip.inc,
// "run rescue"). A rescue slot is one such run; its members are capture indices, in capture order. The representative's cells were saved
// from pass 1's batch into a store laid out as the stream calls' carry store (k_rescue_save), the other members' cells are where pass 2
// left them; rmap[capture] = ~slot or the position in pass 2's batch. Slots at or above *nslots, and slots whose run pass 2 completed
// (gcount 0), return at once.
__global__ __launch_bounds__(256) void k_group_cells_rescue(const uint32_t* __restrict__ plane, Tables tb, const uint8_t* __restrict__ symbols,
                                                            const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                            const uint32_t* __restrict__ flood_flag, const int* __restrict__ gmem,
                                                            const int* __restrict__ gcount, const int* __restrict__ nslots, const int* __restrict__ rmap,
                                                            uint8_t* __restrict__ gsym, uint8_t* __restrict__ gcol, uint16_t* __restrict__ gmargin,
                                                            uint32_t* __restrict__ gdisp, CarryStore cs)
{
	if ((int)blockIdx.y >= *nslots || gcount[blockIdx.y] == 0) return;   // (uniform over the workgroup)
	group_cells_body<false, true>(plane, tb, symbols, colors, drift, flood_flag, gmem, gcount, nslots, gsym, gcol, gmargin, gdisp, cs, rmap);
}

// G4 over the rescue slots. The members' chunks and masks are the call's per-capture outputs, by capture index: k_group_end's addressing, so
// the body is the plain calls' instantiation, writing the slot's row of the staging the Reed-Solomon pass decoded into. Behind it the row
// goes to the run's place: rchunks[run] / rmasks[run] (each may be nullptr) replace what k_repeat_end wrote there, and tap[run] = the bits
// the rescue added to the OR of the members' masks.
__global__ __launch_bounds__(256) void k_group_end_rescue(const uint8_t* __restrict__ gsym, const uint16_t* __restrict__ gmargin, Tables tb,
                                                          const int* __restrict__ gmem, const int* __restrict__ gcount, const int* __restrict__ nslots,
                                                          const uint8_t* __restrict__ grs_ok, const uint8_t* __restrict__ chunks,
                                                          const uint32_t* __restrict__ masks, const uint32_t* __restrict__ gdisp,
                                                          uint8_t* __restrict__ gchunks, uint32_t* __restrict__ gmasks, int e_on, int e_max,
                                                          const int* __restrict__ slot_run, uint8_t* __restrict__ rchunks, uint32_t* __restrict__ rmasks,
                                                          int32_t* __restrict__ tap)
{
	const int g = blockIdx.x;
	if (g >= *nslots || gcount[g] == 0) return;                          // (uniform over the workgroup)
	group_end_body<false>(gsym, gmargin, tb, gmem, gcount, nslots, grs_ok, chunks, masks, gdisp, gchunks, gmasks, e_on, e_max, CarryStore{}, nullptr);
	__syncthreads();                                                      // (the row is whole, and visible to the whole workgroup)
	const int run = slot_run[g];
	if (rchunks) carry_copy(rchunks + (size_t)run * FRAME_BYTES, gchunks + (size_t)g * FRAME_BYTES, FRAME_BYTES);
	if (threadIdx.x == 0) {
		const uint32_t gm = gmasks[g];
		uint32_t mm = 0;
		for (int c = 0; c < gcount[g]; ++c) mm |= masks[gmem[(size_t)g * GMAX + c]];
		if (rmasks) rmasks[run] = gm;
		tap[run] = (int32_t)(gm & ~mm);
	}
}

// ------------------------------------------------------------------------------------------------ tear salvage (the once-calls, opt-in)
// cimbar_hip_set_once_tear_salvage: the rescue's group decode where a torn capture beside the run joins the vote on its good side
// (repeat.hip.inc, "tear salvage"). gcount[slot] counts the full members and the partials, gfull[slot] the full members alone; the slot's
// row of `part` is {kp, axis_p, lo_p, hi_p, kf, axis_f, lo_f, hi_f} and gmem holds the partials behind the full members, in that order. A
// partial takes part in cell i iff lo <= line_axis(i) < hi, line_tab being the stitched calls' table; member 0 is always a full member.
__global__ __launch_bounds__(256) void k_group_cells_salvage(const uint32_t* __restrict__ plane, Tables tb, const uint8_t* __restrict__ symbols,
                                                             const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                             const uint32_t* __restrict__ flood_flag, const int* __restrict__ gmem,
                                                             const int* __restrict__ gcount, const int* __restrict__ gfull,
                                                             const int32_t* __restrict__ part, const uint8_t* __restrict__ line_tab,
                                                             const int* __restrict__ nslots, const int* __restrict__ rmap, uint8_t* __restrict__ gsym,
                                                             uint8_t* __restrict__ gcol, uint16_t* __restrict__ gmargin, uint32_t* __restrict__ gdisp,
                                                             CarryStore cs)
{
	if ((int)blockIdx.y >= *nslots || gcount[blockIdx.y] == 0) return;   // (uniform over the workgroup)
	group_cells_body<false, true, true>(plane, tb, symbols, colors, drift, flood_flag, gmem, gcount, nslots, gsym, gcol, gmargin, gdisp, cs, rmap, gfull, part,
	                                    line_tab);
}
