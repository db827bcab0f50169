// k2b_flood.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K2b: exact flood-order pass
// ------------------------------------------------------------------------------------------------ K2b exact flood
// FloodDecodePositions.cpp:17-134 + CimbReader.cpp:139-162 + CimbDecoder.cpp:101-147, literally: the visiting order of the
// reference's std::priority_queue decides which neighbour's drift a cell inherits, so the queue is replayed operation for
// operation (libstdc++ bits/stl_heap.h push_heap / pop_heap, including how equal priorities fall) -- a serial algorithm.
// One wavefront per flagged frame, everything it touches per step in LDS (the frame's bit plane, per-cell state, the heap),
// and the 64 lanes cooperate inside every step:
//   * heap pop: the walk down the tree fetches a whole 6-level subtree with one gather (lane l <- node r*2^d + l, d = depth
//     of l in the subtree), picks children with v_readlane, and the libstdc++ "hole" shuffle becomes one scattered write;
//   * heap push: the <=17 ancestors of the new slot are fetched with one gather, a ballot finds where the climb stops;
//   * decode: the (window, tile) popcounts are spread over the lanes, DPP min-reduce;
//   * the <=12 neighbour offers (4 adjacent + 8 "horizon") are evaluated one per lane from a precomputed candidate table.
// A heap entry carries everything the reference keeps in _instructions[] for a cell (an accepted offer always has a
// strictly smaller priority than the cell's previous ones, so the entry that pops first IS the latest instruction):
//   prio(7) << 25 | cell(14) << 11 | dx+8 (4) << 7 | dy+8 (4) << 3 | cooldown code (3)
// The eight seed cells are the exception (their seed entry pops with priority 0/1 but must use the latest accepted offer, if
// any): their current instruction lives in s_seed[]. s_state[cell] (u8) = best offered priority + 1, 0x7F (no offer yet), or, once
// visited, 0x80 | symbol. The symbols go out when the frame is done; the position the colour pass reads is one fire-and-forget
// 2-byte store per step (nothing in the loop waits for stores: the only loads are the two prefetches, consumed a pop later).
#ifndef CIMBAR_HEAP_LDS
#define CIMBAR_HEAP_LDS 10240
#endif
constexpr int HEAP_LDS = CIMBAR_HEAP_LDS;  // heap slots held in LDS (40 KiB; a clean shifted frame peaks near 9 200 live entries); deeper slots
                                 // spill to the global scratch under the same indices (tests build a second library with
                                 // CIMBAR_HEAP_LDS=1024 so that the spill path runs on ordinary frames)
struct FloodScratch {
	uint32_t* heap;      // [areas][HEAP_CAP] one spill area per workgroup; only indices >= HEAP_LDS are ever touched
	uint32_t* next;      // [FLOOD_COUNTERS] one counter PAIR per launch that may be in flight (the host zeroes the pair in stream order in front of every launch that uses it, host.hip.inc launch_exact_flood): workgroups take frames as they finish
	uint8_t* prio;       // [areas][PRIO_STRIDE] k_flood3's dense instance: the per-cell "best offered priority + 1" bytes (everything else of s_state is in LDS bits)
};
constexpr int PRIO_STRIDE = (NCELLS + 16 + 255) / 256 * 256;
// (FLOOD_COUNTERS: chainplan.hip.inc)

__device__ __forceinline__ uint32_t cool_enc(uint32_t c) { return c == 0xFEu ? 0u : (c == 0xFFu ? 2u : c); }   // real values: 1,3,4,5,7
__device__ __forceinline__ uint32_t cool_dec(uint32_t k) { return k == 0u ? 0xFEu : (k == 2u ? 0xFFu : k); }

typedef __attribute__((address_space(3))) uint32_t lds_u32;
// The spill half of the heap (slots >= HEAP_LDS, global memory), only compiled into the SPILL = true instance of a step
// (taken when the heap is within a step's growth of HEAP_LDS). Out of line on purpose: it is cold, and inlined the compiler
// would have to assume pending global loads around every heap access.
template <int HEAP_N>
__device__ __attribute__((noinline)) uint32_t heap_spill_get(const uint32_t* g, int i, uint32_t v) { return i >= HEAP_N ? g[i] : v; }
template <int HEAP_N>
__device__ __attribute__((noinline)) void heap_spill_set(uint32_t* g, int i, uint32_t v, bool on) { if (on && i >= HEAP_N) g[i] = v; }

// the lane mask of a predicate. (__ballot() goes through v_cndmask 0 / 1 + v_cmp_ne even when the predicate already IS a lane mask in scalar
// registers: two vector instructions per ballot, in a chain where every instruction is ~5 cycles)
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

struct PopPrefetch { uint32_t value, v, vl, vr; };

// LEVEL (k_flood3's dense instance): HEAP_N = 64^k - 1, i.e. the LDS holds whole six-level blocks of the tree (k = 2: levels 0..11) and every deeper
// level lives in `glob`. The spill accessors are then inline -- a lane mask and a branch that is not taken while no lane's slot is deep -- because in
// this instance half of all camera frames spend a good part of their replay with a heap larger than the LDS part (oracle/ co_last_heap_peak:
// 2 600 .. 6 600 live entries), where the out-of-line accessors of the other instances (a call per access) made a pop three times as long.
template <int HEAP_N, bool LEVEL = false>   // heap slots held in LDS; deeper ones live in `glob` (SPILL instances only)
struct WaveHeap {
	lds_u32* lds;
	uint32_t* glob;
	int n;
	// per lane, for pop(): lane l = node l + 1 of a 63-node subtree (1 = its root); bit (p - 1) of ancm is set for every proper ancestor p of
	// that node, and in dirm as well where the path from p towards the node goes into p's RIGHT child
	unsigned long long ancm = 0, dirm = 0;
	__device__ __forceinline__ void lanes(int lane)
	{
		ancm = 0; dirm = 0;
		if (lane >= 1 && lane < 63) {
			const unsigned node = (unsigned)lane + 1u;
			for (unsigned c = node; c > 1u; c >>= 1) {
				const unsigned p = c >> 1;
				ancm |= 1ull << (p - 1u);
				if (c & 1u) dirm |= 1ull << (p - 1u);
			}
		}
	}
	// i, on: per lane. Reads are unconditional (a masked-off lane reads slot 0) so that they cost no branch.
	template <bool SPILL>
	__device__ __forceinline__ uint32_t get(int i, bool on = true) const
	{
		uint32_t v = lds[(on && i < HEAP_N) ? i : 0];
		if constexpr (SPILL && LEVEL) {
			const bool deep = on && i >= HEAP_N;
			if (ballot64(deep)) { if (deep) v = glob[i]; }
		} else if constexpr (SPILL) v = heap_spill_get<HEAP_N>(glob, on ? i : 0, v);
		return v;
	}
	template <bool SPILL>
	__device__ __forceinline__ void set(int i, uint32_t v, bool on) const
	{
		if (on && i < HEAP_N) lds[i] = v;
		if constexpr (SPILL && LEVEL) { if (on && i >= HEAP_N) glob[i] = v; }
		else if constexpr (SPILL) heap_spill_set<HEAP_N>(glob, i, v, on);
	}

	// std::push_heap after push_back (stl_heap.h __push_heap): climb while the parent's priority is greater
	template <bool SPILL>
	__device__ __forceinline__ void push(uint32_t e, int lane)
	{
		const int pos = n++;
		const int depth = 31 - __builtin_clz((unsigned)pos + 1u);        // ancestors a_1 .. a_depth (= root)
		const int a = (int)(((unsigned)pos + 1u) >> (lane < 31 ? lane : 31)) - 1;   // a_0 = pos
		const bool anc = lane >= 1 && lane <= depth;
		const uint32_t v = get<SPILL>(a, anc);
		const unsigned long long stop = ballot64((v >> 25) <= (e >> 25)) & ((2ull << depth) - 2ull);   // (lanes 1 .. depth: the ancestors)
		const int m = stop ? (int)__builtin_ctzll(stop) - 1 : depth;   // the new element lands in a_m
		const uint32_t vnext = from_right_lane(v, 0u);                   // lane k <- H[a_{k+1}]
		set<SPILL>(a, lane < m ? vnext : e, lane <= m);
	}

	// what pop() reads first, so that it can be requested together with the peek at the top
	template <bool SPILL>
	__device__ __forceinline__ PopPrefetch prefetch(int lane) const
	{
		const int len = n - 1, half = (len - 1) / 2;
		PopPrefetch p;
		p.value = get<SPILL>(len > 0 ? len : 0);
		p.v = get<SPILL>(lane, lane < 63 && lane < len);
		const bool inner = lane < 31 && lane < half;
		p.vl = get<SPILL>(2 * lane + 1, inner);
		p.vr = get<SPILL>(2 * lane + 2, inner);
		return p;
	}

	// std::pop_heap + pop_back (stl_heap.h __pop_heap -> __adjust_heap -> __push_heap); the caller has read the top already.
	// __adjust_heap walks the hole from the root to the bottom, always into the child the comparator prefers (the right one on
	// ties), moving that child up; __push_heap then lifts the old last element `value` back up over the moved elements. In
	// terms of the OLD array and the path c_0 = root, c_1, .., c_L: with j = the deepest k >= 1 whose H[c_k] has priority <=
	// value's (0 if none), H[c_{k-1}] <- H[c_k] for k <= j, H[c_j] <- value, everything else stays.
	// The walk takes five levels per LDS round trip: lane l fetches node l of the 63-node subtree under the hole (global
	// index hole*2^d + l, d = depth of l) and, if it is an inner node, its two children; a ballot turns the comparisons into
	// one bit per node and the descent is five scalar bit-lookups.
	template <bool SPILL>
	__device__ __forceinline__ void pop(int lane, const PopPrefetch& pf)
	{
		const int len = n - 1;                  // elements that remain; `value` = the old last one, re-inserted from the root
		if (len == 0) { n = 0; return; }
		const uint32_t value = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf.value);
		const uint32_t vprio = value >> 25;
		const int half = (len - 1) / 2;         // nodes below this index have two children
		const int d = 31 - __builtin_clz((unsigned)lane + 1u);
		uint32_t bv[4];
		int bg[4];
		bool bp[4];
		int S = 1, depth = 0, j = 0;            // 1-based index of the hole, its depth, and the j of the comment above
#pragma unroll
		for (int B = 0; B < 4; ++B) {
			bv[B] = 0; bg[B] = 0; bp[B] = false;
			if (S - 1 < half) {
				const int gi = ((S - 1) << d) + lane;
				const bool inner = lane < 31 && gi < half;
				uint32_t v, vl, vr;
				if (B == 0) { v = pf.v; vl = pf.vl; vr = pf.vr; }
				else {
					v = get<SPILL>(gi, lane < 63 && gi < len);
					vl = get<SPILL>(2 * gi + 1, inner);
					vr = get<SPILL>(2 * gi + 2, inner);
				}
				// comp(first[second], first[second-1]) -> second-- : the left child only if the right one's priority is greater
				const unsigned long long right = ballot64(inner && !((vr >> 25) > (vl >> 25)));
				const unsigned long long innerm = ballot64(inner);
				// the walk, all lanes at once instead of five dependent scalar steps: a node is on the hole's path iff every ancestor has two
				// children and prefers the child that leads to it
				const bool onp = ancm != 0ull && ((right ^ dirm) & ancm) == 0ull && (innerm & ancm) == ancm;
				const unsigned long long pm = ballot64(onp);
				if (pm) {
					const int last = 63 - (int)__builtin_clzll(pm);            // the deepest node reached (breadth-first numbering: the highest lane)
					S = __builtin_amdgcn_readlane(gi, last) + 1;
					depth += (int)__popcll(pm);
				}
				const bool onpath = (pm >> lane) & 1ull;
				bv[B] = v; bg[B] = gi; bp[B] = onpath;
				const unsigned long long cm = ballot64(onpath && (v >> 25) <= vprio);
				if (cm) j = 5 * B + (31 - __builtin_clz((unsigned)(63 - (int)__builtin_clzll(cm)) + 1u));
			}
		}
		// (four blocks cover 20 levels; HEAP_CAP < 2^18)
		int tail = -1;                              // a last node with a left child only
		uint32_t tailv = 0;
		if ((len & 1) == 0 && S - 1 == (len - 2) / 2) {
			tail = 2 * (S - 1) + 1;
			tailv = (uint32_t)__builtin_amdgcn_readfirstlane((int)get<SPILL>(tail));
			++depth;
			if ((tailv >> 25) <= vprio) j = depth;
		}
#pragma unroll
		for (int B = 0; B < 4; ++B) {
			if (B == 0 || 5 * B < depth) {
				const int dp = 5 * B + d;
				set<SPILL>((bg[B] - 1) >> 1, bv[B], bp[B] && dp <= j);
				set<SPILL>(bg[B], value, bp[B] && dp == j);
			}
		}
		if (tail >= 0 && j == depth) {
			set<SPILL>((tail - 1) >> 1, tailv, lane == 0);
			set<SPILL>(tail, value, lane == 0);
		}
		if (j == 0) set<SPILL>(0, value, lane == 0);
		n = len;
	}
};

__device__ __forceinline__ uint32_t calc_cooldown(uint32_t previous, uint32_t idx)
{
	// CellDrift.cpp:33-43
	if (idx == 4) return 4;
	if ((idx & 1) == 0) return 0xFF;
	if (((previous ^ idx) & 0xFF) == 6) return 0xFF;
	return idx;
}

// minimum of a 32-bit value over the wave (uniform result). (`old` = 0xFFFFFFFF, the identity of an unsigned minimum -- every lane has a source under these
// controls, so it is never used -- lets the compiler fold each cross-lane move into the v_min itself: v_min_u32_dpp, one instruction per step instead of
// v_mov + v_mov_dpp + v_min behind a wait state)
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
	uint32_t o;
	o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0xB1, 0xf, 0xf, false); v = o < v ? o : v;    // quad_perm:[1,0,3,2]
	o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x4E, 0xf, 0xf, false); v = o < v ? o : v;    // quad_perm:[2,3,0,1]
	o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x141, 0xf, 0xf, false); v = o < v ? o : v;   // row_half_mirror
	o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x140, 0xf, 0xf, false); v = o < v ? o : v;   // row_mirror
	const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
	const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), e = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
	const uint32_t ab = a < b ? a : b, ce = c < e ? c : e;
	return ab < ce ? ab : ce;
}

// FloodDecodePositions.cpp:27-41, in push order; -1 for everything else. All eight sit in the first 712 or last 712 cells.
__device__ __forceinline__ int seed_slot(int i)
{
	if ((unsigned)(i - (TOP_CELLS + DIM_X)) < (unsigned)(NCELLS - 2 * (TOP_CELLS + DIM_X))) return -1;
	int s = -1;
	s = i == 0 ? 0 : s;
	s = i == TOP_W - 1 ? 1 : s;
	s = i == NCELLS - 1 ? 2 : s;
	s = i == NCELLS - TOP_W ? 3 : s;
	s = i == TOP_CELLS ? 4 : s;
	s = i == TOP_CELLS + DIM_X - 1 ? 5 : s;
	s = i == NCELLS - 1 - TOP_CELLS ? 6 : s;
	s = i == NCELLS - TOP_CELLS - DIM_X ? 7 : s;
	return s;
}

// One step of the exact replay = one decoded cell (FloodDecodePositions::next + CimbReader::read + FloodDecodePositions::update), run by
// one wavefront. State it works on: the LDS heap, s_state / s_seed as described at the top of this file, the frame's bit plane and the
// offer table. Returns false when the heap ran empty. Shared by k_flood (the whole frame) and k_flood_wave (its exact prefix).
struct FloodLane {
	int lane;
	uint64_t my_tile;
	uint32_t h_cs, h_r8;
};
__device__ __forceinline__ FloodLane flood_lane_init(int lane)
{
	FloodLane fl;
	fl.lane = lane;
	fl.my_tile = c_tile[lane & 15];
	// lanes 0..8 each build the 8x8 hash of window w = lane out of the ten 10-bit rows (bit_extractor.h:23-51)
	const int hw = lane < 9 ? lane : 0;
	fl.h_cs = 2u - (uint32_t)(hw % 3);
	fl.h_r8 = 8u * (uint32_t)(hw / 3);
	return fl;
}
constexpr uint32_t FLOOD_DEFAULT_D = (8u << 7) | (8u << 3) | 0u;              // CellDrift(), cooldown 0xFE
constexpr uint32_t FLOOD_ORDER8 = 0x20813754u;   // nibble k = k-th window visited: 4,5,7,3,1,8,0,2 and then 6 (ahash_result.h:26)

#ifdef FLOOD_PROF
#define PROF_T0() pc0 = __builtin_readcyclecounter()
#define PROF_ADD(k) do { unsigned long long pc1 = __builtin_readcyclecounter(); pt[k] += pc1 - pc0; pc0 = pc1; } while (0)
#else
#define PROF_T0()
#define PROF_ADD(k)
#endif

template <bool SPILL, int HEAP_N>
__device__ __forceinline__ bool flood_step(WaveHeap<HEAP_N>& hp, uint8_t* s_state, uint32_t* s_seed, const uint32_t* __restrict__ pl,
                                           const Tables& tb, int8_t* __restrict__ drift_frame, const FloodLane& fl
#ifdef FLOOD_PROF
                                           , unsigned long long* pt
#endif
)
{
	const int lane = fl.lane;
#ifdef FLOOD_PROF
	unsigned long long pc0;
#endif
	PROF_T0();
	// ---- FloodDecodePositions::next(): pop until a cell that still needs decoding turns up. The top of the heap names
	// the cell, and (with s_seed) where its window is, before the pop has run: the twenty bit-plane words of the
	// window and the cell's offer list are requested from L2 first and arrive behind the pop.
	int i = -1;
	uint32_t e = 0, di = 0, prev_prio = 0, pw = 0, sh = 0;
	int16_t cand = -1;
	while (hp.n > 0) {
		const uint32_t topv = hp.template get<SPILL>(0);
		const PopPrefetch pf = hp.template prefetch<SPILL>(lane);   // same LDS round trip as the peek
		e = (uint32_t)__builtin_amdgcn_readfirstlane((int)topv);
		PROF_ADD(7);
		const int idx = (int)((e >> 11) & 0x3FFFu);
		const bool fresh = ((uint32_t)__builtin_amdgcn_readfirstlane((int)s_state[idx]) & 0x80u) == 0;
		if (fresh) {
			di = e & 0x7FFu; prev_prio = e >> 25;
			const int slot = seed_slot(idx);
			if (slot >= 0) { const uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_seed[slot]); di = sv & 0x7FFu; prev_prio = sv >> 16; }
			// CellPositions.cpp:5-51 (the three bands of mode B)
			int cx, cy;
			if (idx < TOP_CELLS) { cx = OFFSET + (MARKER + idx % TOP_W) * PITCH; cy = OFFSET + (idx / TOP_W) * PITCH; }
			else if (idx < TOP_CELLS + MID_CELLS) { const int q = idx - TOP_CELLS; cx = OFFSET + (q % DIM_X) * PITCH; cy = OFFSET + (MARKER + q / DIM_X) * PITCH; }
			else { const int q = idx - TOP_CELLS - MID_CELLS; cx = OFFSET + (MARKER + q % TOP_W) * PITCH; cy = OFFSET + (DIM_Y - MARKER + q / TOP_W) * PITCH; }
			const int x0 = cx + (int)(di >> 7) - 9, y0 = cy + (int)((di >> 3) & 15u) - 9;   // top-left of the 10x10 window
			const int j = x0 >> 5, j1 = j + 1 > 31 ? 31 : j + 1;   // j == 31: the window ends inside word 31
			sh = 54u - (uint32_t)(x0 & 31);
			// lane 2r: first word of window row r, lane 2r+1: the next word
			if (lane < 20) pw = pl[(y0 + (lane >> 1)) * 32 + ((lane & 1) ? j1 : j)];
			if (lane < 12) cand = tb.cand[(size_t)idx * 12 + lane];
		}
		PROF_ADD(8);
		hp.template pop<SPILL>(lane, pf);
#ifdef FLOOD_PROF
		pt[4] += 1;
		if ((unsigned long long)hp.n > pt[6]) pt[6] = hp.n;
#endif
		if (!fresh) continue;
		i = idx;
		break;
	}
	if (i < 0) return false;
	PROF_ADD(0);
	const int ddx = (int)(di >> 7) - 8, ddy = (int)((di >> 3) & 15u) - 8;
	const uint32_t cooldown = cool_dec(di & 7u);

	// even lanes < 20 form their 10-bit row (MSB = leftmost pixel); the rows become wave-uniform through readlane, and
	// lane w < 9 assembles window w's hash: byte k = bits [cs, cs+8) of row r0+k, r0 = w/3, cs = 2 - w%3
	//   -> the 10 bytes packed big-endian, cut at byte r0
	uint32_t hlo, hhi;
	{
		const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pw, 0xB1, 0xf, 0xf, true);   // quad_perm:[1,0,3,2]: lane^1
		const uint32_t row = (uint32_t)((((uint64_t)pw << 32) | nxt) >> sh);
		uint32_t tb_[10];
#pragma unroll
		for (int r = 0; r < 10; ++r) tb_[r] = ((uint32_t)__builtin_amdgcn_readlane((int)row, 2 * r) >> fl.h_cs) & 0xFFu;
		const uint32_t W0 = (tb_[0] << 24) | (tb_[1] << 16) | (tb_[2] << 8) | tb_[3];
		const uint32_t W1 = (tb_[4] << 24) | (tb_[5] << 16) | (tb_[6] << 8) | tb_[7];
		const uint32_t W2 = (tb_[8] << 24) | (tb_[9] << 16);
		const uint64_t A = (((uint64_t)W0 << 32) | W1) << fl.h_r8;
		hhi = (uint32_t)(A >> 32);
		hlo = (uint32_t)A | ((W2 >> 16) >> (16u - fl.h_r8));
	}

	// (window position k in visiting order, tile t) pairs over the lanes; key = dist << 8 | k << 4 | t, min wins
	const int nwin = (cooldown == 0xFEu) ? 9 : 5;         // CimbDecoder.cpp:144
	uint32_t best = 0xFFFFFFFFu;
#pragma unroll
	for (int it = 0; it < 3; ++it) {
		if (it * 4 >= nwin) break;
		const int k = (lane >> 4) + 4 * it;
		const uint32_t w = k < 8 ? (FLOOD_ORDER8 >> (4 * k)) & 15u : 6u;
		const uint32_t wlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)hlo);
		const uint32_t whi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)hhi);
		const bool skip = k >= nwin || (w == cooldown && w != 4u);   // CimbDecoder.cpp:114-115
		const uint32_t d = (uint32_t)__popc(wlo ^ (uint32_t)fl.my_tile) + (uint32_t)__popc(whi ^ (uint32_t)(fl.my_tile >> 32));
		const uint32_t key = skip ? 0xFFFFFFFFu : ((d << 8) | ((uint32_t)k << 4) | (uint32_t)(lane & 15));
		best = key < best ? key : best;
	}
	best = wave_min(best);
	PROF_ADD(1);

	const uint32_t kbest = (best >> 4) & 15u;
	const uint32_t error_distance = best >> 8, w = kbest < 8 ? (FLOOD_ORDER8 >> (4 * kbest)) & 15u : 6u, bits = best & 15u;
	const int bdx = (int)(w % 3) - 1, bdy = (int)(w / 3) - 1;                 // CellDrift.h:13-15
	int ndx = ddx + bdx, ndy = ddy + bdy;                                     // CellDrift.cpp:23-31
	ndx = ndx > 7 ? 7 : (ndx < -7 ? -7 : ndx);
	ndy = ndy > 7 ? 7 : (ndy < -7 ? -7 : ndy);
	const uint32_t ncool = calc_cooldown(cooldown, w);
	// visited + the symbol; the position the colour pass reads (CimbReader.cpp:158-160 pos.x/y) goes straight to memory
	if (lane == 0) {
		s_state[i] = (uint8_t)(0x80u | bits);
		*reinterpret_cast<uint16_t*>(drift_frame + (size_t)i * 2) =
		    (uint16_t)(((uint32_t)(ddx + bdx) & 0xFFu) | (((uint32_t)(ddy + bdy) & 0xFFu) << 8));
	}

	// ---- FloodDecodePositions::update(): lanes 0-3 the adjacent cells (right, left, bottom, top), 4-7 the horizontal
	// "horizon" (:93-111), 8-11 the vertical one (:113-129), in the reference's offer order. No cell occurs twice in
	// one list (checked when the table is built), so the twelve update_adjacents checks are independent.
	const unsigned long long have = ballot64(cand >= 0);
	const bool far = prev_prio < 3 && error_distance < 3 && cooldown == 4 && ncool == 4;
	const uint32_t lanes_ok = 0xFu | (far && (have & 3ull) == 3ull ? 0xF0u : 0u) | (far && (have & 12ull) == 12ull ? 0xF00u : 0u);
	const bool want = lane < 12 && ((lanes_ok >> (lane & 15)) & 1u) && cand >= 0;
	// update_adjacents (:69-83): still to decode and strictly better than what the cell was offered before
	const uint32_t cst = s_state[want ? (int)cand : 0];
	const bool accept = want && !(cst & 0x80u) && cst >= error_distance + 2u;
	const uint32_t dcode = ((uint32_t)(ndx + 8) << 7) | ((uint32_t)(ndy + 8) << 3) | cool_enc(ncool);
	if (accept) {
		s_state[cand] = (uint8_t)(error_distance + 1u);
		const int sl = seed_slot((int)cand);
		if (sl >= 0) s_seed[sl] = (error_distance << 16) | dcode;
	}
	unsigned long long acc = ballot64(accept);
	PROF_ADD(2);
	while (acc) {
		const int q = (int)__builtin_ctzll(acc);
		acc &= acc - 1;
		const uint32_t cell = (uint32_t)__builtin_amdgcn_readlane((int)cand, q);
		hp.template push<SPILL>((error_distance << 25) | (cell << 11) | dcode, lane);
#ifdef FLOOD_PROF
		pt[5] += 1;
#endif
	}
	PROF_ADD(3);
	return true;
}

// fresh per-frame state + the eight seeds (FloodDecodePositions.cpp:17-42), by one wavefront; the caller brackets it with barriers
template <class HP>
__device__ __forceinline__ void flood_reset(HP& hp, uint8_t* s_state, uint32_t* s_seed, int lane, int nlanes)
{
	uint4 ff; ff.x = ff.y = ff.z = ff.w = 0x7F7F7F7Fu;
	for (int i = lane; i < (NCELLS + 16) / 16; i += nlanes) reinterpret_cast<uint4*>(s_state)[i] = ff;
	if (lane < 8) s_seed[lane] = (0xFEu << 16) | FLOOD_DEFAULT_D;
}
template <class HP>
__device__ __forceinline__ void flood_seed(HP& hp, int lane)
{
	const uint32_t last = NCELLS - 1;
	auto seed = [&](uint32_t prio, uint32_t cell) { hp.template push<false>((prio << 25) | (cell << 11) | FLOOD_DEFAULT_D, lane); };
	seed(0, 0u); seed(0, (uint32_t)(TOP_W - 1)); seed(0, last); seed(0, last - (TOP_W - 1));
	seed(1, (uint32_t)TOP_CELLS); seed(1, (uint32_t)(TOP_CELLS + DIM_X - 1)); seed(1, last - TOP_CELLS); seed(1, last - (TOP_CELLS + DIM_X - 1));
}

// Two instances: HEAP_LDS slots in LDS (52 KiB with the state: three workgroups per CU, 768 frames resident) for batches that fit, and
// HEAP_LDS4 slots (just under 40 KiB: four per CU, 1024 resident; a clean shifted frame then spends part of its life in the spill path) for larger
// ones, where a second round of the 24 ms kernel would cost more than the spilling does. (The launch sizes that go with them, FLOOD_GRID3, FLOOD_GRID
// and the dense instance's FLOOD_DENSE_PER, are chainplan.hip.inc's.)
#ifndef CIMBAR_HEAP_LDS4
#define CIMBAR_HEAP_LDS4 7080
#endif
constexpr int HEAP_LDS4 = HEAP_LDS < CIMBAR_HEAP_LDS4 ? HEAP_LDS : CIMBAR_HEAP_LDS4;   // four workgroups per CU: 4 x (12 416 state + 28 320 heap + 200 seeds / messages) <= 160 KiB
// ... and the dense instance (k_flood3<.., true>: visited BITS in LDS, priorities in global memory, levels 0..11 of the heap in LDS): 1 552 + 4 x 4 096 + 192 = 18 128 bytes, eight
// workgroups per CU (2 048 frames resident, four wavefronts per SIMD) with 13 KiB of every CU's LDS left for another stream's kernels
#ifndef CIMBAR_HEAP_LDS8
#define CIMBAR_HEAP_LDS8 4095
#endif
constexpr int HEAP_LDS8 = HEAP_LDS < CIMBAR_HEAP_LDS8 ? 63 : CIMBAR_HEAP_LDS8;   // (the spill-test build: one block in LDS, every deeper access global)
// flood_flag[f]: 0 = the parallel pass (k_symbols) was exact; 1 = needs the exact replay; 2 = settled by k_flood_wave; 3 = flooded in rounds by
// k_flood_rounds (k2d_floodrounds.hip.inc; only with cimbar_hip_set_relaxed_flood on -- k_rounds_check may set it back to 1). Whoever reads the
// flag to learn "does this frame have drift?" tests != 0.
//
// The replay kernel is k_flood3 below. Its two predecessors are gone (round 4): k_flood, one wavefront per frame running flood_step above
// for all 12 400 cells (24-34 ms per frame: ~620 dependent instructions per step), and k_flood2, which split the step over two wavefronts
// (pop | decode + offers) with two workgroup barriers per step (17.9 ms per frame). flood_step itself stays: it is k_flood_wave's exact prefix.

// ---- k_flood3: the exact replay, two wavefronts per frame with ONE rendezvous per step.
// A lone wavefront retires a dependent instruction every 4-5 cycles, and the two halves of a step do not depend on each other: the pop needs only
// the heap, the decode of the popped cell only the TOP ENTRY, which is known before the pop runs. Wavefront H owns the heap (pops, pushes),
// wavefront D decodes and decides the offers. A naive hand-over (pop || decode -> barrier -> pushes, publish the new top -> barrier -> both
// re-read it) puts four LDS round trips and a barrier of pure hand-over on the heap owner's chain. They are not needed:
//   * after its pop, H knows the heap's new root R and size n (registers);
//   * D knows the offers O it accepted (registers);
//   * the entry that will be on top once O has been pushed follows from R and O alone: all offers of a step carry the same priority ed;
//     the first one climbs to the root iff every ancestor's priority is greater, i.e. iff ed < prio(R) (the root is the minimum), and no
//     later one passes it (equal priorities do not pass, stl_heap.h __push_heap). So top' = ed < prio(R) or n == 0 ? first offer : R.
// Both wavefronts exchange (R, n) and O at the single barrier and then BOTH compute top' (checked against the CPU replay on every step of
// the test frames: no exception). H runs pushes(k) and pop(k+1) back to back, D decodes the cell of top' meanwhile, and whether that entry
// is stale is D's business alone (it owns s_state). The sequence of heap operations is the reference's, operation for operation.
// The pop takes SIX heap levels per LDS round trip (every lane of the 63-node subtree fetches its two children, the next subtree hangs
// under the chosen child of the deepest node) -- two rounds instead of three for the 2 000 .. 4 000 live entries of a camera frame's flood.
// pop7: six levels per round, written for instruction count (the heap owner's chain is what bounds a step, and two thirds of it is the pop:
// every instruction saved here is ~7 cycles off ~20 000 steps per frame). Against the five-level WaveHeap::pop above:
//   * every node on the hole's path writes ONE slot -- its own: H'[c_k] = H[c_(k+1)] for k < j (the value of the child the path goes to, which
//     the lane has fetched anyway: vl or vr), H'[c_j] = value; the root (the hole) is an ordinary path node: no write to a parent's slot, none
//     across blocks, no "if (j == 0)" special case;
//   * a node with a left child only (stl_heap.h __adjust_heap's `(len & 1) == 0 && secondChild == (len - 2) / 2` case) is just a node that
//     "prefers" its only child: the path condition becomes "every ancestor HAS the child that leads here and prefers it", and the tail case
//     with its extra LDS round trip is gone;
//   * reads are unconditional with clamped addresses (what an out-of-range lane fetches is never used), predicates are lane masks.
// tools/heap_model.cpp models exactly this (levels = 7) against std::push_heap / std::pop_heap.
template <int HEAP_N, bool LEVEL = false>
struct WaveHeap7 : WaveHeap<HEAP_N, LEVEL> {
	static_assert(!LEVEL || HEAP_N == 63 || HEAP_N == 4095, "the LDS part of a LEVEL heap ends where a six-level block of the pop ends");
	using WaveHeap<HEAP_N, LEVEL>::n;
	using WaveHeap<HEAP_N, LEVEL>::ancm;
	using WaveHeap<HEAP_N, LEVEL>::dirm;
	using WaveHeap<HEAP_N, LEVEL>::lds;
	using WaveHeap<HEAP_N, LEVEL>::glob;
	int d7 = 0, lane_big = 0;            // depth of this lane's node in a 63-node subtree; the lane number, or something huge for lane 63 (it has no node)
	__device__ __forceinline__ void lanes7(int lane)
	{
		this->lanes(lane);
		d7 = 31 - __builtin_clz((unsigned)lane + 1u);
		lane_big = lane < 63 ? lane : 0x20000000;
	}
	template <bool SPILL>
	__device__ __forceinline__ uint32_t fetch(int i) const
	{
		if constexpr (SPILL && LEVEL) return this->template get<true>(i, (unsigned)i < (unsigned)n);   // (no global round trip for slots that hold nothing)
		else if constexpr (SPILL) return this->template get<true>(i, (unsigned)i < (unsigned)HEAP_CAP);
		else return lds[(unsigned)i < (unsigned)HEAP_N ? i : HEAP_N - 1];
	}
	// push4: up to four pushes of ONE priority (a step's offers all carry the decoded cell's distance) with one gather and one scatter instead of
	// one LDS round trip each. std::push_heap only touches the ancestors of the new last element, so appending all k entries first and then
	// sifting them up in order passes through the same heap states. Lane 16 g + t keeps the CURRENT value of node ((n + g + 1) >> t) - 1, the
	// level-t ancestor of entry g's slot (t = 0: the slot itself), through the k sift-ups: sift-up p moves the values on its path down by one as
	// far as level m_p (the first ancestor whose current priority is not greater stops it, stl_heap.h __push_heap) and puts e_p there; every lane
	// whose node lies on that path -- in whichever group -- takes its new value from the lane above it, which tracks the same parent.
	// `mine` = the entry of this lane's group. Needs n >= 4 (no entry's ancestor is another new entry) and n + 4 <= 32767 (at most 14
	// ancestors); the caller pushes one by one otherwise. tools/heap_model.cpp: push4, same name.
	__device__ __forceinline__ bool push4_ok() const { return n >= 4 && n + 4 <= 32767; }
	template <bool SPILL>
	__device__ __forceinline__ void push4(uint32_t mine, int k, int lane)
	{
		const uint32_t ed = mine >> 25;
		const int g = lane >> 4, t = lane & 15;
		const unsigned pos1 = (unsigned)(n + g) + 1u;
		const int depth = 31 - __builtin_clz(pos1);
		const bool on = g < k && t <= depth;
		const int a = (int)(pos1 >> t) - 1;
		const int dcn = depth - t;
		const uint32_t got = this->template get<SPILL>(a, on && t > 0);
		uint32_t cur = t == 0 ? mine : got;
		const uint32_t orig = cur;
		// (lanes of the k groups that hold an ancestor: t = 1 .. depth of their group's slot; one comparison per ballot, see pop7)
		const unsigned long long cand = ballot64(t <= depth) & 0xFFFEFFFEFFFEFFFEull & (k >= 4 ? ~0ull : ((1ull << (16 * k)) - 1ull));
#pragma unroll
		for (int p = 0; p < 4; ++p) {
			if (p < k) {
				const unsigned pp1 = (unsigned)(n + p) + 1u;
				const int pdepth = 31 - __builtin_clz(pp1);
				const uint32_t ep = (uint32_t)__builtin_amdgcn_readlane((int)mine, 16 * p);
				const unsigned stop = (unsigned)((ballot64((cur >> 25) <= ed) & cand) >> (16 * p)) & 0xFFFFu;
				const int m = stop ? (int)__builtin_ctz(stop) - 1 : pdepth;
				const uint32_t up = from_right_lane(cur, 0u);
				const int kk = pdepth - dcn;
				const bool onpath = on && (unsigned)kk <= (unsigned)m && (int)(pp1 >> (kk & 31)) - 1 == a;
				cur = onpath ? (kk < m ? up : ep) : cur;
			}
		}
		this->template set<SPILL>(a, cur, on && (t == 0 || cur != orig));
		n += k;
	}

	// both children of node (i - 1) / 2, i.e. slots i and i + 1: one clamped address, one ds_read2_b32
	template <bool SPILL>
	__device__ __forceinline__ void fetch_pair(int i, uint32_t& a, uint32_t& b) const
	{
		if constexpr (SPILL && LEVEL) {
			// (i is odd: a left child. Both slots are on the same side of the LDS / global boundary, HEAP_N being odd)
			const int c = (unsigned)i < (unsigned)(HEAP_N - 1) ? i : HEAP_N - 2;
			a = lds[c];
			b = lds[c + 1];
			const bool deep = i >= HEAP_N && i < n;
			if (ballot64(deep)) { if (deep) { a = glob[i]; b = i + 1 < n ? glob[i + 1] : 0u; } }      // (no right child: nothing read past the live heap -- nor past the spill area when n == HEAP_CAP)
		} else if constexpr (SPILL) { a = fetch<true>(i); b = fetch<true>(i + 1); }
		else {
			const int c = (unsigned)i < (unsigned)(HEAP_N - 1) ? i : HEAP_N - 2;
			a = lds[c];
			b = lds[c + 1];
		}
	}
	struct Prefetch7 { uint32_t value, v, vl, vr; };
	template <bool SPILL>
	__device__ __forceinline__ Prefetch7 prefetch7() const
	{
		Prefetch7 p;
		p.value = fetch<SPILL>(n > 1 ? n - 1 : 0);
		p.v = fetch<SPILL>(lane_big);
		fetch_pair<SPILL>(2 * lane_big + 1, p.vl, p.vr);
		return p;
	}
	// returns the root the heap has afterwards (undefined when it ran empty)
	// pop7 for a LEVEL heap that reaches (or may reach) below its LDS part. The same walk and the same writes; what differs is WHEN things are asked for:
	//   * the re-inserted element `value` may come out of global memory, and all it decides is j -- how far down it sinks -- not the path: the comparisons
	//     against its priority are made after the walk, so its round trip runs under the walk's own;
	//   * a block that consists of one leaf (the usual case one level below the LDS part: 4 095 < n <= 8 191) has nothing to fetch: the leaf's value is
	//     the child its parent block has in registers.
	// A pop then costs ONE global round trip (the children of the last LDS level) on top of the LDS-only pop.
	__device__ __forceinline__ uint32_t pop7_deep(const Prefetch7& pf)
	{
		const int len = n - 1;
		if (len == 0) { n = 0; return 0u; }
		uint32_t bchild[3], bv[3];
		unsigned long long bpm[3];
		int bg[3];
		bool bp[3];
		int r0 = 0;
		bool cont = true;
		uint32_t rootchild = 0, vpass = 0;
#pragma unroll
		for (int B = 0; B < 3; ++B) {
			bg[B] = 0; bchild[B] = 0; bp[B] = false; bv[B] = 0; bpm[B] = 0ull;
			if (cont) {
				const int gi = (r0 << d7) + lane_big;
				const int cl = 2 * gi + 1;
				uint32_t v, vl, vr;
				if (B == 0) { v = pf.v; vl = pf.vl; vr = pf.vr; }
				else if (2 * r0 + 1 >= len) { v = vpass; vl = 0u; vr = 0u; }     // (uniform) the block's root has no child: lane 0 is all there is
				else { v = fetch<true>(gi); fetch_pair<true>(cl, vl, vr); }
				const bool two = cl + 1 < len, pref = (vr >> 25) <= (vl >> 25);
				const bool rsel = two & pref;
				const unsigned long long contm = ballot64(cl < len);
				const unsigned long long right = ballot64(two) & ballot64(pref);
				const unsigned long long bad = ((right ^ dirm) & ancm) | (~contm & ancm);
				const bool onp = (bad == 0ull) & (lane_big < 63);
				const unsigned long long pm = ballot64(bad == 0ull) & 0x7FFFFFFFFFFFFFFFull;
				bg[B] = gi; bp[B] = onp; bv[B] = v; bpm[B] = pm;
				bchild[B] = rsel ? vr : vl;
				if (B == 0) rootchild = (uint32_t)__builtin_amdgcn_readfirstlane((int)bchild[0]);
				const unsigned long long go = pm & contm & 0x7FFFFFFF80000000ull;
				if (go) {
					const int gl = (int)__builtin_ctzll(go);
					r0 = __builtin_amdgcn_readlane(cl + (rsel ? 1 : 0), gl);
					vpass = (uint32_t)__builtin_amdgcn_readlane((int)bchild[B], gl);
				} else cont = false;
			}
		}
		const uint32_t value = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf.value);
		const uint32_t vprio = value >> 25;
		int j = 0;
#pragma unroll
		for (int B = 0; B < 3; ++B) {
			const unsigned long long cm = ballot64((bv[B] >> 25) <= vprio) & bpm[B];
			if (cm) j = 6 * B + __builtin_amdgcn_readlane(d7, 63 - (int)__builtin_clzll(cm));
		}
#pragma unroll
		for (int B = 0; B < 3; ++B) {
			if (B == 0 || 6 * B <= j) {
				const int dp = 6 * B + d7;
				this->template set<true>(bg[B], dp < j ? bchild[B] : value, bp[B] && dp <= j);
			}
		}
		n = len;
		return j == 0 ? value : rootchild;
	}
	template <bool SPILL>
	__device__ __forceinline__ uint32_t pop7(const Prefetch7& pf)
	{
		if constexpr (SPILL && LEVEL) return pop7_deep(pf);
		const int len = n - 1;
		if (len == 0) { n = 0; return 0u; }
		const uint32_t value = (uint32_t)__builtin_amdgcn_readfirstlane((int)pf.value);
		const uint32_t vprio = value >> 25;
		uint32_t bchild[3];
		int bg[3];
		bool bp[3];
		int r0 = 0, j = 0;
		bool cont = true;
		uint32_t rootchild = 0;
#pragma unroll
		for (int B = 0; B < 3; ++B) {
			bg[B] = 0; bchild[B] = 0; bp[B] = false;
			if (cont) {
				const int gi = (r0 << d7) + lane_big;
				const int cl = 2 * gi + 1;
				uint32_t v, vl, vr;
				if (B == 0) { v = pf.v; vl = pf.vl; vr = pf.vr; }
				else { v = fetch<SPILL>(gi); fetch_pair<SPILL>(cl, vl, vr); }
				// (every ballot is the ballot of ONE comparison, combined in scalar registers: the ballot of an AND of two comparisons costs a
				// v_cndmask 0 / 1 + v_cmp_ne pair on top)
				const bool two = cl + 1 < len, pref = (vr >> 25) <= (vl >> 25);
				const bool rsel = two & pref;                                            // has two children and prefers the right one (ties go right)
				const unsigned long long contm = ballot64(cl < len);                      // has a (left) child
				const unsigned long long right = ballot64(two) & ballot64(pref);
				const unsigned long long bad = ((right ^ dirm) & ancm) | (~contm & ancm);   // some ancestor lacks the child that leads here, or prefers the other
				const bool onp = (bad == 0ull) & (lane_big < 63);
				const unsigned long long pm = ballot64(bad == 0ull) & 0x7FFFFFFFFFFFFFFFull;   // (lane 63 carries no node)
				const unsigned long long cm = ballot64((v >> 25) <= vprio) & pm;
				bg[B] = gi; bp[B] = onp;
				bchild[B] = rsel ? vr : vl;
				if (B == 0) rootchild = (uint32_t)__builtin_amdgcn_readfirstlane((int)bchild[0]);
				if (cm) j = 6 * B + __builtin_amdgcn_readlane(d7, 63 - (int)__builtin_clzll(cm));      // (the deepest such node: the highest lane)
				// the path leaves the block through its node on the block's last level (lanes 31 .. 62), if that node has a child: into the child it prefers
				const unsigned long long go = pm & contm & 0x7FFFFFFF80000000ull;
				if (go) r0 = __builtin_amdgcn_readlane(cl + (rsel ? 1 : 0), (int)__builtin_ctzll(go));
				else cont = false;
			}
		}
		// (three blocks cover 18 levels; HEAP_CAP < 2^18)
#pragma unroll
		for (int B = 0; B < 3; ++B) {
			if (B == 0 || 6 * B <= j) {
				const int dp = 6 * B + d7;
				this->template set<SPILL>(bg[B], dp < j ? bchild[B] : value, bp[B] && dp <= j);
			}
		}
		n = len;
		return j == 0 ? value : rootchild;
	}
};

// message slots (u32), double-buffered by step parity: D -> H [0] offers accepted, [1] their priority, [2] their drift / cooldown code,
// [3] cells decoded so far, [4..15] the cells in offer order; H -> D [16] the heap's root after the pop, [17] entries left
constexpr int FM_N = 0, FM_ED = 1, FM_DC = 2, FM_DONE = 3, FM_CELLS = 4, FM_ROOT = 16, FM_LEFT = 17, FM_WORDS = 18;

// GSTATE (the dense instance: twice the frames per CU): the per-cell byte array leaves the LDS. What the heap owner needs of it -- "has this cell been
// decoded?" -- is one BIT per cell (1.5 KiB, s_state reinterpreted as words); the offered priorities, which only the decoding wavefront reads and writes,
// live in global memory (sc.prio, one area per workgroup: its own stores and loads, in program order), requested right behind the offer list so that the
// round trip runs under the decode; the symbol goes straight to `symbols` when the cell is decoded.
template <int HEAP_N, bool GSTATE>
__global__ __launch_bounds__(128) void k_flood3(const uint32_t* __restrict__ plane, Tables tb, FloodScratch sc,
                                                const uint32_t* __restrict__ flood_flag, uint8_t* __restrict__ symbols,
                                                int8_t* __restrict__ drift, int f0, int nframes, int area0, int counter)
{
	constexpr int VIS_WORDS = (NCELLS + 31) / 32;
	__shared__ __attribute__((aligned(16))) uint8_t s_state[GSTATE ? (VIS_WORDS * 4 + 15) / 16 * 16 : NCELLS + 16];
	uint32_t* const s_vis = reinterpret_cast<uint32_t*>(s_state);
	// has the cell been decoded? (per lane or uniform)
	auto visited = [&](int cell) -> bool {
		if constexpr (GSTATE) return (s_vis[cell >> 5] >> (cell & 31)) & 1u;
		else return (s_state[cell] & 0x80u) != 0;
	};
	__shared__ uint32_t s_heap[(HEAP_N + 3) / 4 * 4];
	__shared__ uint32_t s_seed[8];
	__shared__ uint32_t s_msg[2][FM_WORDS + 2];
	__shared__ int s_next;
	const int lane = threadIdx.x & 63;
	const bool isH = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
	const FloodLane fl = flood_lane_init(lane);
	// the heap owner is the critical path of every step and shares its SIMD with another frame's decoder wavefront (four frames per CU: one
	// owner and one decoder per SIMD): it gets the issue slots first
	if (isH) __builtin_amdgcn_s_setprio(3);

	// A workgroup's first frame is its block index; where the launch has more frames than workgroups the rest are handed out by a counter: a replay
	// takes 15 .. 30 ms depending on the frame, and with a fixed frame list per workgroup the launch would end with a few workgroups working through
	// their lists alone. (No counter traffic at all when every frame has its own workgroup -- the clean-batch case, where this kernel only looks at
	// the flags.) The host zeroes the counter pair in front of every such launch; the last workgroup to leave zeroes it as well (belt and braces).
	const bool dyn = (int)gridDim.x < nframes;
	uint32_t* const ctr = sc.next + 2 * counter;
	int fi = 0;
	for (bool first = true;; first = false) {
		__syncthreads();   // the previous frame of this workgroup is completely done with the LDS (and everyone has read s_next)
		if (first) fi = (int)blockIdx.x;
		else {
			if (!dyn) break;
			if (threadIdx.x == 0) s_next = (int)gridDim.x + (int)atomicAdd(ctr, 1u);
			__syncthreads();
			fi = s_next;
		}
		if (fi >= nframes) break;
		const int f = f0 + fi;
		if (flood_flag[f] != 1u) continue;
		const uint32_t* pl = plane + (size_t)f * PLANE_WORDS;
		int8_t* drift_frame = drift + (size_t)f * NCELLS * 2;
		WaveHeap7<HEAP_N, GSTATE> hp;
		hp.lds = (lds_u32*)s_heap; hp.glob = sc.heap + (size_t)(area0 + blockIdx.x) * HEAP_CAP; hp.n = 0;
		hp.lanes7(lane);
		uint8_t* const prio = GSTATE ? sc.prio + (size_t)(area0 + blockIdx.x) * PRIO_STRIDE : nullptr;
		uint8_t* const sym_frame = symbols + (size_t)f * NCELLS;
		if constexpr (GSTATE) {
			for (int i = (int)threadIdx.x; i < VIS_WORDS; i += 128) s_vis[i] = 0u;
			if (threadIdx.x < 8) s_seed[threadIdx.x] = (0xFEu << 16) | FLOOD_DEFAULT_D;
			if (!isH) {   // the decoding wavefront is the only one that ever touches the priorities
				uint4 ff; ff.x = ff.y = ff.z = ff.w = 0x7F7F7F7Fu;
				for (int i = lane; i < PRIO_STRIDE / 16; i += 64) reinterpret_cast<uint4*>(prio)[i] = ff;
			}
		} else flood_reset(hp, s_state, s_seed, (int)threadIdx.x, 128);
		__syncthreads();
		if (isH) {
			flood_seed(hp, lane);
			const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_heap[0]);
			if (lane == 0) { s_msg[0][FM_ROOT] = r; s_msg[0][FM_LEFT] = (uint32_t)hp.n; }
		} else if (lane < 4) s_msg[0][lane] = 0u;
		__syncthreads();
#ifdef FLOOD_PROF
		unsigned long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		unsigned long long pc0 = __builtin_readcyclecounter();
#endif
		int decoded = 0;                                 // D's count (H reads it from the message)
		// every pop is one iteration and there are at most as many pops as pushes: the bound only guards against a bug turning into a hang
		for (int k = 0; k < HEAP_CAP + 16; ++k) {
			const int par = k & 1;
			const uint32_t m = s_msg[par][lane < FM_WORDS ? lane : 0];
			const uint32_t nacc = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_N), ed = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_ED);
			const uint32_t dc = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_DC), done = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_DONE);
			const uint32_t root = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_ROOT), left = (uint32_t)__builtin_amdgcn_readlane((int)m, FM_LEFT);
			if (left + nacc == 0u || done >= (uint32_t)NCELLS) break;
			const bool first = nacc > 0u && (left == 0u || ed < (root >> 25));
			const uint32_t e = first ? ((ed << 25) | ((uint32_t)__builtin_amdgcn_readlane((int)m, FM_CELLS) << 11) | dc) : root;
			PROF_ADD(0);                                   // H: hand-over; D: hand-over
			if (isH) {
				const bool stale_e = visited((int)((e >> 11) & 0x3FFFu));     // (D marked it before the barrier if it ever did)
				// FloodDecodePositions::update()'s pushes of the step before, then next(): the pop of the entry on top -- which is `e`
				for (uint32_t q = 0; q < nacc;) {
					if (hp.push4_ok()) {
						// four at a time: lane 16 g + t works on offer q + g
						const uint32_t k4 = nacc - q < 4u ? nacc - q : 4u;
						const uint32_t cell = (uint32_t)__builtin_amdgcn_ds_bpermute((FM_CELLS + (int)q + (lane >> 4)) << 2, (int)m);
						const uint32_t mine = (ed << 25) | (cell << 11) | dc;
						if (hp.n + 16 <= HEAP_N) hp.template push4<false>(mine, (int)k4, lane);
						else hp.template push4<true>(mine, (int)k4, lane);
						q += k4;
					} else {
						const uint32_t entry = (ed << 25) | ((uint32_t)__builtin_amdgcn_readlane((int)m, FM_CELLS + (int)q) << 11) | dc;
						if (hp.n + 16 <= HEAP_N) hp.template push<false>(entry, lane);
						else hp.template push<true>(entry, lane);
						++q;
					}
				}
				PROF_ADD(1);
				// A stale entry (its cell was decoded through a better offer) makes D do nothing: no offers, no state written. Then the next
				// entry on top is simply the new root, and whether THAT one is stale is in s_state as well -- H keeps popping on its own until
				// the root is a cell D has to look at (FloodDecodePositions.cpp's `continue`), and only then goes to the rendezvous.
				uint32_t r = e;
				bool stale = __builtin_amdgcn_readfirstlane((int)stale_e) != 0;
				for (bool own = false;; own = true) {
					const bool spill = hp.n + 16 > HEAP_N;
					if (!spill) {
						const auto pf = hp.template prefetch7<false>();
						if (own && !__builtin_amdgcn_readfirstlane((int)visited((int)((r >> 11) & 0x3FFFu)))) break;
						r = hp.template pop7<false>(pf);
					} else {
						const auto pf = hp.template prefetch7<true>();
						if (own && !__builtin_amdgcn_readfirstlane((int)visited((int)((r >> 11) & 0x3FFFu)))) break;
						r = hp.template pop7<true>(pf);
					}
	#ifdef FLOOD_PROF
					pt[7] += own ? 1 : 0;
	#endif
					if (!stale || hp.n == 0) break;
				}
				if (lane == 0) { s_msg[par ^ 1][FM_ROOT] = r; s_msg[par ^ 1][FM_LEFT] = (uint32_t)hp.n; }
				PROF_ADD(2);
			} else {
				const int idx = (int)((e >> 11) & 0x3FFFu);
				const bool st_e = visited(idx);                      // (requested first; looked at after the loads below have been issued)
				uint32_t di = e & 0x7FFu, prev_prio = e >> 25;
				const int slot = seed_slot(idx);
				if (slot >= 0) { const uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_seed[slot]); di = sv & 0x7FFu; prev_prio = sv >> 16; }
				// The window and the offer list are requested before it is known whether the entry is stale (any heap entry names a real
				// cell and a drift within the limit, so the addresses are good either way): the L2 round trip starts ~150 cycles earlier.
				// CellPositions.cpp:5-51 (the three bands of the grid)
				int cx, cy;
				if (idx < TOP_CELLS) { cx = OFFSET + (MARKER + idx % TOP_W) * PITCH; cy = OFFSET + (idx / TOP_W) * PITCH; }
				else if (idx < TOP_CELLS + MID_CELLS) { const int q = idx - TOP_CELLS; cx = OFFSET + (q % DIM_X) * PITCH; cy = OFFSET + (MARKER + q / DIM_X) * PITCH; }
				else { const int q = idx - TOP_CELLS - MID_CELLS; cx = OFFSET + (MARKER + q % TOP_W) * PITCH; cy = OFFSET + (DIM_Y - MARKER + q / TOP_W) * PITCH; }
				const int x0 = cx + (int)(di >> 7) - 9, y0 = cy + (int)((di >> 3) & 15u) - 9;   // top-left of the 10x10 window
				const int jw = x0 >> 5, j1 = jw + 1 > 31 ? 31 : jw + 1;
				const uint32_t sh = 54u - (uint32_t)(x0 & 31);
				uint32_t pw = 0;
				int16_t cand = -1;
				if (GSTATE && lane < 12) cand = tb.cand[(size_t)idx * 12 + lane];     // (first: the priorities' addresses hang on it)
				if (lane < 20) pw = pl[(y0 + (lane >> 1)) * PLANE_ROW + ((lane & 1) ? j1 : jw)];
				if (!GSTATE && lane < 12) cand = tb.cand[(size_t)idx * 12 + lane];
				uint32_t gprio = 0;
				if constexpr (GSTATE) gprio = prio[cand >= 0 ? (int)cand : 0];         // needed after the decode: the round trip runs under it
				const bool fresh = __builtin_amdgcn_readfirstlane((int)st_e) == 0;
				uint32_t out_n = 0;
				if (fresh) {
					const int ddx = (int)(di >> 7) - 8, ddy = (int)((di >> 3) & 15u) - 8;
					const uint32_t cooldown = cool_dec(di & 7u);
					uint32_t hlo, hhi;
					{
						const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pw, 0xB1, 0xf, 0xf, true);   // lane^1
						PROF_ADD(3);                               // D: the window has arrived
						const uint32_t row = (uint32_t)((((uint64_t)pw << 32) | nxt) >> sh);
						uint32_t tb_[10];
#pragma unroll
						for (int r = 0; r < 10; ++r) tb_[r] = ((uint32_t)__builtin_amdgcn_readlane((int)row, 2 * r) >> fl.h_cs) & 0xFFu;
						const uint32_t W0 = (tb_[0] << 24) | (tb_[1] << 16) | (tb_[2] << 8) | tb_[3];
						const uint32_t W1 = (tb_[4] << 24) | (tb_[5] << 16) | (tb_[6] << 8) | tb_[7];
						const uint32_t W2 = (tb_[8] << 24) | (tb_[9] << 16);
						const uint64_t A = (((uint64_t)W0 << 32) | W1) << fl.h_r8;
						hhi = (uint32_t)(A >> 32);
						hlo = (uint32_t)A | ((W2 >> 16) >> (16u - fl.h_r8));
					}
					const int nwin = (cooldown == 0xFEu) ? 9 : 5;         // CimbDecoder.cpp:144
					uint32_t best = 0xFFFFFFFFu;
#pragma unroll
					for (int it = 0; it < 3; ++it) {
						if (it * 4 >= nwin) break;
						const int kk = (lane >> 4) + 4 * it;
						const uint32_t w = kk < 8 ? (FLOOD_ORDER8 >> (4 * kk)) & 15u : 6u;
						const uint32_t wlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)hlo);
						const uint32_t whi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)hhi);
						const bool skip = kk >= nwin || (w == cooldown && w != 4u);   // CimbDecoder.cpp:114-115
						const uint32_t dd = (uint32_t)__popc(wlo ^ (uint32_t)fl.my_tile) + (uint32_t)__popc(whi ^ (uint32_t)(fl.my_tile >> 32));
						const uint32_t key = skip ? 0xFFFFFFFFu : ((dd << 8) | ((uint32_t)kk << 4) | (uint32_t)(lane & 15));
						best = key < best ? key : best;
					}
					best = wave_min(best);
					const uint32_t kbest = (best >> 4) & 15u;
					const uint32_t error_distance = best >> 8, w = kbest < 8 ? (FLOOD_ORDER8 >> (4 * kbest)) & 15u : 6u, bits = best & 15u;
					const int bdx = (int)(w % 3) - 1, bdy = (int)(w / 3) - 1;                 // CellDrift.h:13-15
					int ndx = ddx + bdx, ndy = ddy + bdy;                                     // CellDrift.cpp:23-31
					ndx = ndx > 7 ? 7 : (ndx < -7 ? -7 : ndx);
					ndy = ndy > 7 ? 7 : (ndy < -7 ? -7 : ndy);
					const uint32_t ncool = calc_cooldown(cooldown, w);
					if (lane == 0) {
						if constexpr (GSTATE) { atomicOr(&s_vis[idx >> 5], 1u << (idx & 31)); sym_frame[idx] = (uint8_t)bits; }
						else s_state[idx] = (uint8_t)(0x80u | bits);
						*reinterpret_cast<uint16_t*>(drift_frame + (size_t)idx * 2) =
						    (uint16_t)(((uint32_t)(ddx + bdx) & 0xFFu) | (((uint32_t)(ddy + bdy) & 0xFFu) << 8));
					}
					// FloodDecodePositions::update(): see flood_step
					const unsigned long long have = ballot64(cand >= 0);
					const bool far = prev_prio < 3 && error_distance < 3 && cooldown == 4 && ncool == 4;
					const uint32_t lanes_ok = 0xFu | (far && (have & 3ull) == 3ull ? 0xF0u : 0u) | (far && (have & 12ull) == 12ull ? 0xF00u : 0u);
					const bool want = lane < 12 && ((lanes_ok >> (lane & 15)) & 1u) && cand >= 0;
					bool accept;
					if constexpr (GSTATE) {
						// (the cell just decoded is never in its own offer list, so the bit set above does not matter here)
						accept = want && !visited(want ? (int)cand : 0) && gprio >= error_distance + 2u;
					} else {
						const uint32_t cst = s_state[want ? (int)cand : 0];
						accept = want && !(cst & 0x80u) && cst >= error_distance + 2u;
					}
					const uint32_t dcode = ((uint32_t)(ndx + 8) << 7) | ((uint32_t)(ndy + 8) << 3) | cool_enc(ncool);
					if (accept) {
						if constexpr (GSTATE) prio[cand] = (uint8_t)(error_distance + 1u);
						else s_state[cand] = (uint8_t)(error_distance + 1u);
						const int sl = seed_slot((int)cand);
						if (sl >= 0) s_seed[sl] = (error_distance << 16) | dcode;
					}
					const unsigned long long acc = ballot64(accept);
					if (accept) s_msg[par ^ 1][FM_CELLS + __popcll(acc & ((1ull << lane) - 1ull))] = (uint32_t)cand;   // in offer order
					out_n = (uint32_t)__popcll(acc);
					++decoded;
					if (lane == 0) { s_msg[par ^ 1][FM_ED] = error_distance; s_msg[par ^ 1][FM_DC] = dcode; }
					PROF_ADD(4);                                   // D: decode + offers
				}
				if (lane == 0) { s_msg[par ^ 1][FM_N] = out_n; s_msg[par ^ 1][FM_DONE] = (uint32_t)decoded; }
			}
			__syncthreads();
			PROF_ADD(5);                                       // waiting for the other wavefront
#ifdef FLOOD_PROF
			pt[6] += 1;
#endif
		}
#ifdef FLOOD_PROF
		if (lane == 0) for (int q = 0; q < 8; ++q) {
			uint32_t* dst = sc.heap + (size_t)(area0 + blockIdx.x) * HEAP_CAP + (isH ? 0 : 16) + 2 * q;
			dst[0] = (uint32_t)pt[q]; dst[1] = q == 6 ? __builtin_amdgcn_s_getreg((31 << 11) | 4) : (uint32_t)(pt[q] >> 32);   // [6]: steps | HW_ID (which SIMD / wave slot / CU this wavefront ran on)
		}
#endif
		__syncthreads();
		if constexpr (!GSTATE) for (int c = (int)threadIdx.x; c < NCELLS; c += 128) {
			const uint32_t v = s_state[c];
			if (v & 0x80u) sym_frame[c] = (uint8_t)(v & 15u);
		}
	}
	if (dyn && threadIdx.x == 0 && atomicAdd(ctr + 1, 1u) == gridDim.x - 1u) { atomicExch(ctr, 0u); atomicExch(ctr + 1, 0u); }
}
