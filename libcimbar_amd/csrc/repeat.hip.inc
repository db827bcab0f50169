// repeat.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace, after stitch.hip.inc).
// R1-R8: repeat-capture skipping -- a run of captures that show one displayed frame is decoded once, the rest only if that decode is incomplete
// ------------------------------------------------------------------------------------------------ the rule
// A camera films the display faster than it changes, so every frame arrives as a run of near-identical captures. The combined calls find such
// runs from the DECODED cells; cimbar_hip_decode_batch_once / _scan_extract_decode_batch_once_fmt find them in front of the decode, from a
// signature of the ink colours that needs no symbol, no drift and no colour matrix (modes 68 / 67 / 66: four palette colours on black):
//   sums       cell c of a frame, nominal top-left (x, y) = cell_xy[c]: R_c, G_c, B_c = the channel sums over pixel rows y + 2 .. y + 5 and
//              columns x .. x + 7 (32 pixels), S_c = R_c + G_c + B_c. Rows 3..4 alone would not do: some tiles have no ink there.
//   totals     R_A, B_A, S_A = the sums of R_c, B_c, S_c over the frame's NCELLS cells
//   sig_c      [R_c S_A > S_c R_A] | [B_c S_A > S_c B_A] << 1 -- "redder than the frame" and "bluer than the frame"; strict, unsigned 64 bit
//              (the products stay below 2^43). The frame is read as handed in, or as the warp wrote it: sharpening plays no part.
//   agree      agree(k, k + 1) = the cells with equal sig
//   runs       k_group_walk's walk (combine.hip.inc) over that agree array: capture k starts a run when it is the first, when
//              agree(k - 1, k) * 1000 < min_agree_permille * NCELLS, when the run before it already has max_run members, or when capture
//              k - 1 or k is unusable (capture path: extraction failed). An unusable capture is in no run.
//   rep        member (len - 1) / 2 of a run: the first of two, the second of three or four
//   pass 1     the representatives, gathered in capture order, through enqueue() as one plain batch
//   pass 2     the other members of every run whose representative's mask is not full, likewise; no such member: no second pass
//   per run    rmask = the OR of the members' masks; chunk j from the representative where it delivered it, else from the lowest-index
//              member that did, else zeros
//   R1 k_repeat_sums     (cell rows x frames) workgroups: the four needed pixel rows of a cell row, 16 bytes per lane, through LDS to (R, S, B)
//   R2 k_repeat_sig      one workgroup per frame: the totals by a fixed-order block reduction (no atomics), then sig, one byte per cell
//   R3 k_repeat_agree    one workgroup per adjacent pair
//   G2 k_group_walk      as it is
//   R4 k_repeat_lists    roles and list 1 (the representatives) from the walk's members; R5 k_repeat_lists2: list 2 from list 1's masks
//   R6 k_repeat_gather   listed frames (capture path: and their scan status, for the per-frame sharpen choice) into a context-owned buffer
//   R7 k_repeat_clear / k_repeat_scatter   zeroes for what no pass has decoded yet; a pass's chunks and masks back into capture slots
//   R8 k_repeat_end      the per-run fill
// The host reads the length of list 1, and then of list 2, back to size the decode launches (host.hip.inc, once_impl).
// The once-stream calls carry the last capture's run from call to call: "runs across calls" below. Opt-in, the plain once-calls decode a
// run that stays incomplete after pass 2 once more from all its members' cells: "run rescue" below; "tear skipping" leaves torn boundary
// captures undecoded, and "tear salvage", at the end of this file, lets the ones that are decoded vote in that rescue.
constexpr int RP_AGREE_DEFAULT = 900, RP_RUN_DEFAULT = 4;
constexpr int RP_ROW0 = 2, RP_ROWS = 4;                                  // pixel rows y + 2 .. y + 5 of a cell
constexpr int RP_ROW_BYTES = IMG_W * 3, RP_ROW_VEC = RP_ROW_BYTES / 16;   // 3072 | 2208 bytes: 192 | 138 16-byte loads
constexpr int RP_LOADS = (RP_ROWS * RP_ROW_VEC + 255) / 256;             // per lane: 3
static_assert(RP_ROW_BYTES % 16 == 0 && FRAME_RGB % 16 == 0, "pixel rows start on 16-byte boundaries");
static_assert(2 * DIM_X <= 256, "two lanes per cell of a cell row");
static_assert(OFFSET + PITCH * (DIM_Y - 1) + RP_ROW0 + RP_ROWS <= IMG_H && OFFSET + PITCH * (DIM_X - 1) + 8 <= IMG_W, "the last cell's rows and columns lie inside the frame");

enum { RP_ROLE_UNUSABLE = CIMBAR_HIP_ONCE_UNUSABLE, RP_ROLE_SKIPPED = CIMBAR_HIP_ONCE_SKIPPED, RP_ROLE_REP = CIMBAR_HIP_ONCE_REPRESENTATIVE, RP_ROLE_FALLBACK = CIMBAR_HIP_ONCE_FALLBACK };

// R1: workgroup (cr, f) reads pixel rows OFFSET + PITCH cr + 2 .. + 5 of frame f whole -- 4 x RP_ROW_VEC coalesced 16-byte loads -- into LDS;
// then lanes 2c and 2c + 1 sum two of the four rows of grid column c each. sums[f][cell] = {R, S, B, 0}, by linear cell index; the grid
// slots inside the corner cut-outs (grid_cell < 0) are dropped.
__global__ __launch_bounds__(256) void k_repeat_sums(const uint8_t* __restrict__ rgb, Tables tb, ushort4* __restrict__ sums)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_px[RP_ROWS][RP_ROW_BYTES];
	const int cr = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
	const uint8_t* frame = rgb + (size_t)f * FRAME_RGB + (size_t)(OFFSET + PITCH * cr + RP_ROW0) * RP_ROW_BYTES;
	uint4 v[RP_LOADS];
#pragma unroll
	for (int i = 0; i < RP_LOADS; ++i) {
		const int idx = t + 256 * i;
		if (idx < RP_ROWS * RP_ROW_VEC) v[i] = reinterpret_cast<const uint4*>(frame)[idx];   // (the four rows are consecutive in memory)
	}
#pragma unroll
	for (int i = 0; i < RP_LOADS; ++i) {
		const int idx = t + 256 * i;
		if (idx < RP_ROWS * RP_ROW_VEC) reinterpret_cast<uint4*>(&s_px[0][0])[idx] = v[i];
	}
	__syncthreads();
	const int c = t >> 1, h = t & 1;
	uint32_t r = 0, g = 0, b = 0;
	if (c < DIM_X) {
		const int x0 = (OFFSET + PITCH * c) * 3;
#pragma unroll
		for (int row = 0; row < 2; ++row) {
			const uint8_t* p = &s_px[2 * h + row][x0];
#pragma unroll
			for (int px = 0; px < 8; ++px) { r += p[3 * px]; g += p[3 * px + 1]; b += p[3 * px + 2]; }
		}
	}
	r += __shfl_xor(r, 1); g += __shfl_xor(g, 1); b += __shfl_xor(b, 1);
	if (c < DIM_X && h == 0) {
		const int cell = tb.grid_cell[cr * DIM_X + c];
		if (cell >= 0) sums[(size_t)f * NCELLS + cell] = make_ushort4((unsigned short)r, (unsigned short)(r + g + b), (unsigned short)b, 0);
	}
}

// R2: one workgroup per frame. The totals are sums of integers below 2^29 in a fixed order; sig[f][cell] in 0..3.
__global__ __launch_bounds__(256) void k_repeat_sig(const ushort4* __restrict__ sums, uint8_t* __restrict__ sig)
{
	const int f = blockIdx.x;
	const ushort4* s = sums + (size_t)f * NCELLS;
	uint32_t r = 0, t = 0, b = 0;
	for (int c = threadIdx.x; c < NCELLS; c += 256) { const ushort4 v = s[c]; r += v.x; t += v.y; b += v.z; }
	for (int o = 32; o >= 1; o >>= 1) { r += __shfl_xor(r, o); t += __shfl_xor(t, o); b += __shfl_xor(b, o); }
	__shared__ uint32_t s_part[3][4];
	if ((threadIdx.x & 63) == 0) { s_part[0][threadIdx.x >> 6] = r; s_part[1][threadIdx.x >> 6] = t; s_part[2][threadIdx.x >> 6] = b; }
	__syncthreads();
	const unsigned long long RA = (unsigned long long)s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
	const unsigned long long SA = (unsigned long long)s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
	const unsigned long long BA = (unsigned long long)s_part[2][0] + s_part[2][1] + s_part[2][2] + s_part[2][3];
	for (int c = threadIdx.x; c < NCELLS; c += 256) {
		const ushort4 v = s[c];
		const uint32_t red = (unsigned long long)v.x * SA > (unsigned long long)v.y * RA ? 1u : 0u;
		const uint32_t blue = (unsigned long long)v.z * SA > (unsigned long long)v.y * BA ? 2u : 0u;
		sig[(size_t)f * NCELLS + c] = (uint8_t)(red | blue);
	}
}

// R3: one workgroup per pair (k, k + 1), k < n - 1: the cells with equal sig
__global__ __launch_bounds__(256) void k_repeat_agree(const uint8_t* __restrict__ sig, int n, uint32_t* __restrict__ agree)
{
	const int k = blockIdx.x;
	if (k + 1 >= n) return;
	const uint32_t* a = reinterpret_cast<const uint32_t*>(sig + (size_t)k * NCELLS);
	const uint32_t* b = a + NCELLS / 4;
	uint32_t cnt = 0;
	for (int w = threadIdx.x; w < NCELLS / 4; w += 256) {
		const uint32_t x = a[w] ^ b[w];
		cnt += ((x & 0xFFu) == 0u) + ((x & 0xFF00u) == 0u) + ((x & 0xFF0000u) == 0u) + ((x >> 24) == 0u);
	}
	for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
	__shared__ uint32_t s_part[4];
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0) agree[k] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// the representative of run r: member (len - 1) / 2
__device__ __forceinline__ int repeat_rep(const int* __restrict__ rmem, const int* __restrict__ rcount, int r) { return rmem[(size_t)r * GMAX + (rcount[r] - 1) / 2]; }

// R4: one lane per capture. roles[k] = -1 in no run, 1 the representative of its run, else 0; list1[r] = the representative of run r (the runs
// are numbered in capture order, so list 1 is in capture order too)
__global__ __launch_bounds__(256) void k_repeat_lists(const int* __restrict__ runs, const int* __restrict__ rmem, const int* __restrict__ rcount, int n,
                                                      int* __restrict__ roles, int* __restrict__ list1)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const int r = runs[k];
	if (r < 0) { roles[k] = RP_ROLE_UNUSABLE; return; }
	const bool rep = repeat_rep(rmem, rcount, r) == k;
	roles[k] = rep ? RP_ROLE_REP : RP_ROLE_SKIPPED;
	if (rep) list1[r] = k;
}

// R5: one wavefront, 64 captures per step. A skipped capture whose run's representative came back with an incomplete mask (rep_masks[r]: pass
// 1's masks, by run) takes role 2 and joins list 2, in capture order; *count2 = its length. map (the run rescue's, else nullptr): map[k] =
// capture k's position in list 2.
__global__ __launch_bounds__(64) void k_repeat_lists2(const int* __restrict__ runs, const uint32_t* __restrict__ rep_masks, int n, int* __restrict__ roles,
                                                      int* __restrict__ list2, int* __restrict__ count2, int* __restrict__ map)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull;
	constexpr uint32_t FULL = (1u << CHUNKS) - 1u;
	int base = 0;
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		bool take = false;
		if (k < n && roles[k] == RP_ROLE_SKIPPED) take = (rep_masks[runs[k]] & FULL) != FULL;
		const unsigned long long tb = __ballot(take);
		if (take) {
			const int pos = base + (int)__popcll(tb & below);
			roles[k] = RP_ROLE_FALLBACK;
			list2[pos] = k;
			if (map) map[k] = pos;
		}
		base += (int)__popcll(tb);
	}
	if (lane == 0) *count2 = base;
}

// R6: frame list[j] -> dst frame j, j = blockIdx.y; sel_out[j] = that capture's scan status (status == nullptr: none)
__global__ __launch_bounds__(256) void k_repeat_gather(const uint8_t* __restrict__ rgb, const int* __restrict__ list, uint8_t* __restrict__ dst,
                                                       const int* __restrict__ status, int stride, int* __restrict__ sel_out)
{
	const int j = blockIdx.y, k = list[j];
	const uint4* s = reinterpret_cast<const uint4*>(rgb + (size_t)k * FRAME_RGB);
	uint4* d = reinterpret_cast<uint4*>(dst + (size_t)j * FRAME_RGB);
	constexpr int VEC = (int)(FRAME_RGB / 16);
	for (int i = blockIdx.x * 256 + threadIdx.x; i < VEC; i += gridDim.x * 256) d[i] = s[i];
	if (status && blockIdx.x == 0 && threadIdx.x == 0) sel_out[j] = status[(size_t)k * stride];
}

// R7: one workgroup per capture: everything but a representative is zero until a pass delivers it
__global__ __launch_bounds__(256) void k_repeat_clear(const int* __restrict__ roles, uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks)
{
	const int k = blockIdx.x;
	if (roles[k] == RP_ROLE_REP) return;
	if (threadIdx.x == 0) masks[k] = 0;
	for (int i = threadIdx.x; i < FRAME_BYTES; i += 256) chunks[(size_t)k * FRAME_BYTES + i] = 0;
}

// ... and a pass's results, by list position j = blockIdx.x, into the slots of the captures they belong to
__global__ __launch_bounds__(256) void k_repeat_scatter(const int* __restrict__ list, const uint8_t* __restrict__ src_chunks, const uint32_t* __restrict__ src_masks,
                                                        uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks)
{
	const int j = blockIdx.x, k = list[j];
	if (threadIdx.x == 0) masks[k] = src_masks[j];
	for (int i = threadIdx.x; i < FRAME_BYTES; i += 256) chunks[(size_t)k * FRAME_BYTES + i] = src_chunks[(size_t)j * FRAME_BYTES + i];
}

// R8: one workgroup per run slot r < n; slots at or above *nruns are zero. rchunks / rmasks may each be nullptr.
// (The once-stream calls restate this fill with the carried row in front, in repeat_fill_row below: a change to the rule goes to both.)
__global__ __launch_bounds__(256) void k_repeat_end(const int* __restrict__ rmem, const int* __restrict__ rcount, const int* __restrict__ nruns,
                                                    const uint8_t* __restrict__ chunks, const uint32_t* __restrict__ masks, uint8_t* __restrict__ rchunks,
                                                    uint32_t* __restrict__ rmasks)
{
	const int r = blockIdx.x;
	__shared__ int s_src[CHUNKS];
	const bool live = r < *nruns;
	if (threadIdx.x < CHUNKS) {
		int src = -1;
		if (live) {
			const int cnt = rcount[r], rep = repeat_rep(rmem, rcount, r);
			if ((masks[rep] >> threadIdx.x) & 1u) src = rep;
			else
				for (int m = 0; m < cnt && src < 0; ++m) {
					const int k = rmem[(size_t)r * GMAX + m];
					if ((masks[k] >> threadIdx.x) & 1u) src = k;
				}
		}
		s_src[threadIdx.x] = src;
	}
	__syncthreads();
	if (rmasks && threadIdx.x == 0) {
		uint32_t m = 0;
		if (live) for (int j = 0; j < rcount[r]; ++j) m |= masks[rmem[(size_t)r * GMAX + j]];
		rmasks[r] = m;
	}
	if (!rchunks) return;
	for (int i = threadIdx.x; i < FRAME_BYTES; i += 256) {
		const int src = s_src[i / CHUNK];
		rchunks[(size_t)r * FRAME_BYTES + i] = src >= 0 ? chunks[(size_t)src * FRAME_BYTES + i] : (uint8_t)0;
	}
}

// ------------------------------------------------------------------------------------------------ runs across calls (the once-stream calls)
// cimbar_hip_decode_batch_once_stream / _scan_extract_decode_batch_once_stream_fmt carry the run the last capture of a call belongs to into
// the next call. The carry lives on the device in two slots used in turn (a call reads slot `cur` and k_repeat_carry writes the other):
//   sig     the signature of the call's last capture
//   words   {usable, len, P}: that capture was usable; the members of its run so far, over all calls; the OR of the masks its decoded
//           members delivered. len and P are 0 for an unusable capture; all three are 0 after create and after cimbar_hip_once_stream_reset
//   row     the run's chunk row, filled as rchunks is
// A run's SEGMENT is its members in this call. Run 0 may continue the carried run (cw[RPC_CONT]); then its segment's P is the carried P, every
// other segment's P is 0. List 1 holds the representative of every segment whose P is not full, list 2 the other members of every segment
// with P | (its representative's mask) not full.
//   R3s k_repeat_agree_stream  n rows: agree[0] against the carried signature (0 where the carry is unusable), agree[k] = agree(k - 1, k)
//   G2r k_repeat_walk_stream   k_group_walk's walk seeded with the carried run's length and usable word; the member counts without atomics
//   R4s k_repeat_lists_stream / R5s k_repeat_lists2_stream / R8s k_repeat_end_stream   as R4 / R5 / R8, honouring P and the carried row
//   R9  k_repeat_carry         the new carry, into the other slot
constexpr int RP_CARRY_SIG = (NCELLS + 15) & ~15, RP_CARRY_ROW = (FRAME_BYTES + 15) & ~15;   // slot strides, bytes
enum { RPW_USABLE = 0, RPW_LEN = 1, RPW_P = 2, RP_CARRY_WORDS = 4 };                          // a slot's words
enum { RPC_RUNS = 0, RPC_LEN2 = 1, RPC_CONT = 2, RPC_LEN1 = 3, RP_CALL_WORDS = 4 };           // a call's words: runs, |list 2|, continued, |list 1|
constexpr uint32_t RP_FULL = (1u << CHUNKS) - 1u;
static_assert(NCELLS % 4 == 0, "signatures are compared a word at a time");
struct RepeatCarry {
	uint8_t* sig;      // [2][RP_CARRY_SIG]
	uint32_t* words;   // [2][RP_CARRY_WORDS]
	uint8_t* row;      // [2][RP_CARRY_ROW]
	int cur;           // the slot this call reads
};

// the P of run r's segment
__device__ __forceinline__ uint32_t repeat_seg_p(const RepeatCarry& cy, const int* __restrict__ cw, int r)
{
	return (r == 0 && cw[RPC_CONT]) ? cy.words[cy.cur * RP_CARRY_WORDS + RPW_P] : 0u;
}

// R3s: one workgroup per capture k < n: the cells with equal sig in capture k and its predecessor (k = 0: the carried capture)
__global__ __launch_bounds__(256) void k_repeat_agree_stream(const uint8_t* __restrict__ sig, RepeatCarry cy, uint32_t* __restrict__ agree)
{
	const int k = blockIdx.x;
	const bool live = k > 0 || cy.words[cy.cur * RP_CARRY_WORDS + RPW_USABLE] != 0u;
	const uint32_t* b = reinterpret_cast<const uint32_t*>(sig + (size_t)k * NCELLS);
	const uint32_t* a = k > 0 ? b - NCELLS / 4 : reinterpret_cast<const uint32_t*>(cy.sig + (size_t)cy.cur * RP_CARRY_SIG);
	uint32_t cnt = 0;
	if (live)
		for (int w = threadIdx.x; w < NCELLS / 4; w += 256) {
			const uint32_t x = a[w] ^ b[w];
			cnt += ((x & 0xFFu) == 0u) + ((x & 0xFF00u) == 0u) + ((x & 0xFF0000u) == 0u) + ((x >> 24) == 0u);
		}
	for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
	__shared__ uint32_t s_part[4];
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0) agree[k] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// G2r: one wavefront, 64 captures per step, as k_group_walk (groups_in == nullptr) with these differences. agree has n entries, agree[k]
// against capture k's predecessor. Capture 0 continues the carried run when the carried capture and it are usable, agree[0] reaches the
// threshold and the carried run has fewer than max_run members (cont); the walk then behaves as if that run had started len captures in
// front of capture 0, so that its members of earlier calls count toward max_run. Without cont, capture 0 breaks as the first capture of a
// plain call does. A run's member count is written by the head of the run behind it (the members in front of that head minus those in front
// of the run), the last run's by lane 0 at the end: no atomics, nothing to zero.
//   runs[k], rmem, rcount   as k_group_walk's groups, gmem, gcount, over the members in this call
//   cw                      RPC_RUNS, RPC_CONT, RPC_LEN1 = the runs minus a continued run 0 whose carried P is full, RPC_LEN2 = 0
__global__ __launch_bounds__(64) void k_repeat_walk_stream(const uint32_t* __restrict__ agree, int n, const int* __restrict__ status, int stride,
                                                           int min_agree, int max_run, RepeatCarry cy, int* __restrict__ runs, int* __restrict__ rmem,
                                                           int* __restrict__ rcount, int* __restrict__ cw)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
	const unsigned long long need = (unsigned long long)min_agree * NCELLS;
	const uint32_t* w = cy.words + cy.cur * RP_CARRY_WORDS;
	const bool cu = w[RPW_USABLE] != 0u;
	const int L = cu ? (int)w[RPW_LEN] : 0;
	const bool u0 = !status || status[0] > 0;
	const bool cont = cu && u0 && (unsigned long long)agree[0] * 1000ull >= need && L < max_run;
	int run_carry = cont ? -L : 0, starts_carry = cont ? 1 : 0, mem_carry = 0, base_carry = 0, prev_id = -1, top = -1;
	bool prev_u = cu;
	auto fetch = [&](int k, uint32_t& a, int& st) {
		a = k < n ? agree[k] : 0u;
		st = (status && k < n) ? status[(size_t)k * stride] : 1;
	};
	uint32_t a_cur; int st_cur;
	fetch(lane, a_cur, st_cur);
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		uint32_t a_nxt; int st_nxt;
		fetch(k + 64, a_nxt, st_nxt);
		const bool in = k < n;
		const bool u = in && st_cur > 0;
		const unsigned long long ub = __ballot(u);
		const bool u_prev = lane == 0 ? prev_u : ((ub >> (lane - 1)) & 1ull) != 0;
		const bool brk = in && ((k == 0 && !cont) || !u_prev || (unsigned long long)a_cur * 1000ull < need);
		const unsigned long long bb = __ballot(brk) & upto;
		const int run = bb ? k0 + 63 - __clzll(bb) : run_carry;          // the latest break at or before k (cont: the carried run's virtual start)
		const bool start = u && (k - run) % max_run == 0;
		const unsigned long long sb = __ballot(start);
		const int id = u ? starts_carry + (int)__popcll(sb & upto) - 1 : -1;
		run_carry = __shfl(run, 63);
		starts_carry += (int)__popcll(sb);
		const int id_prev_lane = __shfl(id, lane > 0 ? lane - 1 : 0);
		const int id_prev = lane == 0 ? prev_id : id_prev_lane;
		const bool head = id >= 0 && (k == 0 || id_prev != id);
		const bool member = id >= 0;
		const unsigned long long mb = __ballot(member), hb = __ballot(head) & upto;
		const int before = mem_carry + (int)__popcll(mb & below);           // members of the call in front of capture k
		const int hl = hb ? 63 - __clzll(hb) : lane;
		const int at_head = __shfl(before, hl);
		const int base = hb ? at_head : base_carry;                          // members in front of k's run
		const int base_prev_lane = __shfl(base, lane > 0 ? lane - 1 : 0);
		const int base_prev = lane == 0 ? base_carry : base_prev_lane;       // members in front of the run before k's, where k heads one
		if (in) runs[k] = id;
		if (member) rmem[(size_t)id * GMAX + (before - base)] = k;
		if (head && id > 0) rcount[id - 1] = before - base_prev;
		top = id > top ? id : top;
		prev_id = __shfl(id, 63);
		prev_u = __shfl((int)u, 63) != 0;
		mem_carry += (int)__popcll(mb);
		base_carry = __shfl(base, 63);
		a_cur = a_nxt; st_cur = st_nxt;
	}
	for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(top, o); top = t > top ? t : top; }
	if (lane == 0) {
		if (top >= 0) rcount[top] = mem_carry - base_carry;
		const bool skip0 = cont && (w[RPW_P] & RP_FULL) == RP_FULL;
		cw[RPC_RUNS] = top + 1;
		cw[RPC_LEN2] = 0;
		cw[RPC_CONT] = cont ? 1 : 0;
		cw[RPC_LEN1] = top + 1 - (skip0 ? 1 : 0);
	}
}

// R4s: one lane per capture, as R4; the members of a continued run 0 whose carried P is full are all skipped, and list 1 starts at run 1
__global__ __launch_bounds__(256) void k_repeat_lists_stream(const int* __restrict__ runs, const int* __restrict__ rmem, const int* __restrict__ rcount, int n,
                                                             const int* __restrict__ cw, int* __restrict__ roles, int* __restrict__ list1)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const int r = runs[k];
	if (r < 0) { roles[k] = RP_ROLE_UNUSABLE; return; }
	const int off = cw[RPC_RUNS] - cw[RPC_LEN1];
	const bool rep = r >= off && repeat_rep(rmem, rcount, r) == k;
	roles[k] = rep ? RP_ROLE_REP : RP_ROLE_SKIPPED;
	if (rep) list1[r - off] = k;
}

// R5s: as R5. rep_masks holds pass 1's masks by list position, run r at r - off; run 0's carried P counts as delivered.
__global__ __launch_bounds__(64) void k_repeat_lists2_stream(const int* __restrict__ runs, const uint32_t* __restrict__ rep_masks, int n, RepeatCarry cy,
                                                             int* __restrict__ roles, int* __restrict__ list2, int* __restrict__ cw)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull;
	const int off = cw[RPC_RUNS] - cw[RPC_LEN1];
	int base = 0;
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		bool take = false;
		if (k < n && roles[k] == RP_ROLE_SKIPPED) {
			const int r = runs[k];
			if (r >= off) take = ((rep_masks[r - off] | repeat_seg_p(cy, cw, r)) & RP_FULL) != RP_FULL;
		}
		const unsigned long long tb = __ballot(take);
		if (take) { roles[k] = RP_ROLE_FALLBACK; list2[base + (int)__popcll(tb & below)] = k; }
		base += (int)__popcll(tb);
	}
	if (lane == 0) cw[RPC_LEN2] = base;
}

// The row of run r by one workgroup of 256 (live: r is a run of this call): chunk j from the carried row where the segment's P has bit j, else
// from the representative where it delivered it, else from the lowest-index member that did, else zeros; *out_mask = P | the OR of the
// members' masks. out_row / out_mask may each be nullptr. s_src: CHUNKS ints of LDS.
__device__ __forceinline__ void repeat_fill_row(int r, bool live, const int* __restrict__ rmem, const int* __restrict__ rcount, const uint8_t* __restrict__ chunks,
                                                const uint32_t* __restrict__ masks, const RepeatCarry& cy, const int* __restrict__ cw, uint8_t* __restrict__ out_row,
                                                uint32_t* __restrict__ out_mask, int* s_src)
{
	const uint32_t P = live ? repeat_seg_p(cy, cw, r) : 0u;
	if (threadIdx.x < CHUNKS) {
		int src = -1;
		if (live) {
			const int cnt = rcount[r], rep = repeat_rep(rmem, rcount, r);
			if ((P >> threadIdx.x) & 1u) src = -2;
			else if ((masks[rep] >> threadIdx.x) & 1u) src = rep;
			else
				for (int m = 0; m < cnt && src == -1; ++m) {
					const int k = rmem[(size_t)r * GMAX + m];
					if ((masks[k] >> threadIdx.x) & 1u) src = k;
				}
		}
		s_src[threadIdx.x] = src;
	}
	__syncthreads();
	if (out_mask && threadIdx.x == 0) {
		uint32_t m = P;
		if (live) for (int j = 0; j < rcount[r]; ++j) m |= masks[rmem[(size_t)r * GMAX + j]];
		*out_mask = m;
	}
	if (!out_row) return;
	const uint8_t* carried = cy.row + (size_t)cy.cur * RP_CARRY_ROW;
	// (one workgroup moves the row, so its time is load latency: every load of a lane is issued before its first store, which nothing lets
	// the compiler do across the stores of a plain copy loop)
	constexpr int PER = (FRAME_BYTES + 255) / 256;
	uint8_t v[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const int i = threadIdx.x + 256 * j;
		uint8_t b = 0;
		if (i < FRAME_BYTES) {
			const int src = s_src[i / CHUNK];
			if (src >= 0) b = chunks[(size_t)src * FRAME_BYTES + i];
			else if (src == -2) b = carried[i];
		}
		v[j] = b;
	}
#pragma unroll
	for (int j = 0; j < PER; ++j) {
		const int i = threadIdx.x + 256 * j;
		if (i < FRAME_BYTES) out_row[i] = v[j];
	}
}

// R8s: one workgroup per run slot r < n; slots at or above the run count are zero. rchunks / rmasks may each be nullptr.
__global__ __launch_bounds__(256) void k_repeat_end_stream(const int* __restrict__ rmem, const int* __restrict__ rcount, const int* __restrict__ cw,
                                                           const uint8_t* __restrict__ chunks, const uint32_t* __restrict__ masks, RepeatCarry cy,
                                                           uint8_t* __restrict__ rchunks, uint32_t* __restrict__ rmasks)
{
	const int r = blockIdx.x;
	__shared__ int s_src[CHUNKS];
	repeat_fill_row(r, r < cw[RPC_RUNS], rmem, rcount, chunks, masks, cy, cw, rchunks ? rchunks + (size_t)r * FRAME_BYTES : nullptr, rmasks ? rmasks + r : nullptr, s_src);
}

// R9: one workgroup. The other slot takes the call's last capture: its signature, whether it is in a run, and if so that run's length over
// all calls, its mask and its row (what R8s reports for it).
__global__ __launch_bounds__(256) void k_repeat_carry(const uint8_t* __restrict__ sig, const int* __restrict__ runs, const int* __restrict__ rmem,
                                                      const int* __restrict__ rcount, const int* __restrict__ cw, const uint8_t* __restrict__ chunks,
                                                      const uint32_t* __restrict__ masks, int n, RepeatCarry cy)
{
	const int to = cy.cur ^ 1, r = runs[n - 1];
	__shared__ int s_src[CHUNKS];
	const uint32_t* s = reinterpret_cast<const uint32_t*>(sig + (size_t)(n - 1) * NCELLS);
	uint32_t* d = reinterpret_cast<uint32_t*>(cy.sig + (size_t)to * RP_CARRY_SIG);
	for (int i = threadIdx.x; i < NCELLS / 4; i += 256) d[i] = s[i];
	uint32_t* w = cy.words + to * RP_CARRY_WORDS;
	if (r < 0) {
		if (threadIdx.x == 0) { w[RPW_USABLE] = 0u; w[RPW_LEN] = 0u; w[RPW_P] = 0u; }
		return;
	}
	if (threadIdx.x == 0) {
		w[RPW_USABLE] = 1u;
		w[RPW_LEN] = (uint32_t)(((r == 0 && cw[RPC_CONT]) ? (int)cy.words[cy.cur * RP_CARRY_WORDS + RPW_LEN] : 0) + rcount[r]);
	}
	repeat_fill_row(r, true, rmem, rcount, chunks, masks, cy, cw, cy.row + (size_t)to * RP_CARRY_ROW, w + RPW_P, s_src);
}

// ------------------------------------------------------------------------------------------------ run rescue (the plain once-calls, opt-in)
// cimbar_hip_set_once_rescue. A run whose members have all been decoded and whose masks together are still not full is given up by the rule
// above, although every member's cells were on the device a moment earlier. With the setting on such a run is decoded once more, as one
// group of the combined call (combine.hip.inc G3, k_rs LIVE, G4), from the cells every member's own pass left:
//   qualifies  a run of two or more members whose representative's mask is not full: pass 2 decodes its other members, so afterwards all of
//              its members are decoded. At most min(|list 1|, |list 2|) runs qualify, each owning a member of list 2: the host sizes the
//              store, the group scratch and every grid below from that bound and reads nothing back for it.
//   slot       a qualifying run's rank among them, in run order
//   tried      a qualifying run whose members' masks, after pass 2, are together still not full
//   R10 k_rescue_save    in front of pass 2, which overwrites pass 1's scratch: the representative's symbols, colours, drift, bit plane and
//                        flood word go from pass 1's batch (position = run) to the slot of a store laid out as the stream calls' carry store;
//                        slot_run, the slot's member row, map[representative] = ~slot and the slot count are written too (k_repeat_lists2
//                        wrote map[k] = the position in list 2 for the other members)
//   R11 k_rescue_tried   behind pass 2's scatter: gcount[slot] = the run's members if it is tried, else 0; gdisp[slot] = 0
//   G3r k_group_cells_rescue, k_rs LIVE, G4r k_group_end_rescue (combine.hip.inc), G4r behind R8: a tried run's row replaces R8's
constexpr int RS_PARTS = 4, RS_ARRAYS = 4;

// R10: workgroup (slice, slot). Wavefront 0 of every workgroup walks the runs, 64 per step with a carried base, to the run of its slot (none:
// the slot is at or above the count and the workgroup returns); then one of RS_PARTS slices of one of the four arrays is copied, 16 bytes
// per lane where the ends allow it (carry_copy).
// (POS: tear skipping's form, where run r's representative stands at pos[r] in pass 1's batch instead of at r; SALVAGE: tear salvage's form of
// that, where a torn capture beside the run lets it qualify and joins its member row; see the end of this file, salvage_side included)
__device__ __forceinline__ bool salvage_side(const int32_t* __restrict__ tap, const int* __restrict__ roles, int k, int n, bool p_side, int guard, int& axis,
                                             int& lo, int& hi);
template <bool POS, bool SALVAGE = false>
__device__ __forceinline__ void rescue_save_body(const uint32_t* __restrict__ plane, const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors,
                                                 const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                 const uint32_t* __restrict__ rep_masks, const int* __restrict__ rmem, const int* __restrict__ rcount,
                                                 int nruns, CarryStore cs, int* __restrict__ slot_run, int* __restrict__ smem, int* __restrict__ map,
                                                 int* __restrict__ nslots, const int* __restrict__ pos, const int* __restrict__ roles = nullptr,
                                                 const int32_t* __restrict__ tap = nullptr, int n = 0, int guard = 0, int32_t* __restrict__ parts = nullptr)
{
	const int slot = blockIdx.y;
	__shared__ int s_run;
	if (threadIdx.x < 64) {
		const int lane = threadIdx.x;
		const unsigned long long below = (1ull << lane) - 1ull;
		int base = 0, mine = -1;
		for (int r0 = 0; r0 < nruns; r0 += 64) {
			const int r = r0 + lane;
			bool q;
			if constexpr (SALVAGE) {
				// (a run slot at or above the run count has no members and no pos; a candidate's run has pos -1 and is never tried)
				const int cnt = r < nruns ? rcount[r] : 0, at = cnt >= 1 ? pos[r] : -1;
				q = at >= 0 && (rep_masks[at] & RP_FULL) != RP_FULL;
				if (q && cnt < 2) {
					int ax, lo, hi;
					const int f = rmem[(size_t)r * GMAX];
					q = salvage_side(tap, roles, f - 1, n, false, guard, ax, lo, hi) || salvage_side(tap, roles, f + 1, n, true, guard, ax, lo, hi);
				}
			} else q = r < nruns && rcount[r] >= 2 && (rep_masks[POS ? pos[r] : r] & RP_FULL) != RP_FULL;
			const unsigned long long qb = __ballot(q);
			if (q && base + (int)__popcll(qb & below) == slot) mine = r;
			base += (int)__popcll(qb);
		}
		for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(mine, o); mine = t > mine ? t : mine; }
		if (lane == 0) {
			s_run = mine;
			if (blockIdx.x == 0 && slot == 0) *nslots = base;
		}
	}
	__syncthreads();
	const int r = s_run;
	if (r < 0) return;                                                   // (uniform over the workgroup)
	if (blockIdx.x == 0) {
		const int cnt = rcount[r];
		if constexpr (SALVAGE) {
			// the member row: the full members, then the preceding partial, then the following one, each only while the row has room
			if (threadIdx.x < GMAX) {
				const int t = threadIdx.x, f = rmem[(size_t)r * GMAX], e = rmem[(size_t)r * GMAX + cnt - 1];
				int pa[2], pl[2], ph[2];
				const bool hp = cnt < GMAX && salvage_side(tap, roles, f - 1, n, false, guard, pa[0], pl[0], ph[0]);
				const bool hf = cnt + (hp ? 1 : 0) < GMAX && salvage_side(tap, roles, e + 1, n, true, guard, pa[1], pl[1], ph[1]);
				int k = 0;
				if (t < cnt) k = rmem[(size_t)r * GMAX + t];
				else if (hp && t == cnt) k = f - 1;
				else if (hf && t == cnt + (hp ? 1 : 0)) k = e + 1;
				smem[(size_t)slot * GMAX + t] = k;
				if (t < 2) {
					int32_t* row = parts + (size_t)slot * 8 + 4 * t;
					const bool have = t == 0 ? hp : hf;
					row[0] = have ? (t == 0 ? f - 1 : e + 1) : -1;
					row[1] = have ? pa[t] : -1;
					row[2] = have ? pl[t] : 0;
					row[3] = have ? ph[t] : 0;
				}
			}
		} else if (threadIdx.x < GMAX) smem[(size_t)slot * GMAX + threadIdx.x] = (int)threadIdx.x < cnt ? rmem[(size_t)r * GMAX + threadIdx.x] : 0;
		if (threadIdx.x == 0) {
			slot_run[slot] = r;
			map[repeat_rep(rmem, rcount, r)] = ~slot;
			cs.flood[slot] = flood_flag[POS ? pos[r] : r];
		}
	}
	const int arr = blockIdx.x / RS_PARTS, part = blockIdx.x % RS_PARTS;
	const size_t k = (size_t)(POS ? pos[r] : r);
	const uint8_t* src; uint8_t* dst; size_t bytes;
	switch (arr) {
		case 0: src = symbols + k * NCELLS; dst = cs.symbols + (size_t)slot * CS_CELLS; bytes = NCELLS; break;
		case 1: src = colors + k * NCELLS; dst = cs.colors + (size_t)slot * CS_CELLS; bytes = NCELLS; break;
		case 2: src = reinterpret_cast<const uint8_t*>(drift + k * NCELLS * 2); dst = reinterpret_cast<uint8_t*>(cs.drift + (size_t)slot * CS_DRIFT); bytes = (size_t)NCELLS * 2; break;
		default: src = reinterpret_cast<const uint8_t*>(plane + k * PLANE_WORDS); dst = reinterpret_cast<uint8_t*>(cs.plane + (size_t)slot * CS_PLANE); bytes = (size_t)PLANE_WORDS * 4; break;
	}
	// this workgroup's slice: whole 16-byte units, the last slice takes the rest
	const size_t per = (bytes / RS_PARTS) & ~(size_t)15, lo = per * part, hi = part == RS_PARTS - 1 ? bytes : lo + per;
	carry_copy(dst + lo, src + lo, hi - lo);
}

__global__ __launch_bounds__(256) void k_rescue_save(const uint32_t* __restrict__ plane, const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors,
                                                     const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                     const uint32_t* __restrict__ rep_masks, const int* __restrict__ rmem, const int* __restrict__ rcount,
                                                     int nruns, CarryStore cs, int* __restrict__ slot_run, int* __restrict__ smem, int* __restrict__ map,
                                                     int* __restrict__ nslots)
{
	rescue_save_body<false>(plane, symbols, colors, drift, flood_flag, rep_masks, rmem, rcount, nruns, cs, slot_run, smem, map, nslots, nullptr);
}

// R11: one lane per slot of the `slots` the host sized for. masks: the call's per-capture masks, pass 2's included.
__global__ __launch_bounds__(256) void k_rescue_tried(const int* __restrict__ nslots, int slots, const int* __restrict__ slot_run, const int* __restrict__ smem,
                                                      const int* __restrict__ rcount, const uint32_t* __restrict__ masks, int* __restrict__ gcount,
                                                      uint32_t* __restrict__ gdisp)
{
	const int s = blockIdx.x * 256 + threadIdx.x;
	if (s >= slots) return;
	int m = 0;
	if (s < *nslots) {
		const int cnt = rcount[slot_run[s]];
		uint32_t all = 0;
		for (int j = 0; j < cnt; ++j) all |= masks[smem[(size_t)s * GMAX + j]];
		m = (all & RP_FULL) != RP_FULL ? cnt : 0;
	}
	gcount[s] = m;
	gdisp[s] = 0u;
}

// ------------------------------------------------------------------------------------------------ tear skipping (the plain once-calls, opt-in)
// cimbar_hip_set_once_tear_skip. A camera that films faster than the display changes catches a frame switch in about one capture of four:
// frame P on one side of a line, frame N on the other. Such a capture agrees with each neighbour on about 600 permille of its cells, so by
// the rule above it is a run of one, its own representative, and decoded in pass 1 -- through the flood path, for chunks its neighbour runs
// already have. With the setting on it is recognised from the signatures and left undecoded where both neighbour runs come back complete:
//   eligible   capture k, 1 <= k <= n - 2, captures k - 1, k, k + 1 usable, k's run has one member
//   lines      line(i), L and width(l) of stitch.hip.inc: axis 0 the grid rows, axis 1 the grid columns; axis 2 evaluates both
//   per line   cntP(l) = the cells of line l whose sig equals capture k - 1's, cntN(l) the same against capture k + 1's;
//              flagP(l) = cntP(l) * 1000 >= line_permille * width(l), flagN(l) likewise; p(l) = flagP & !flagN, q(l) = flagN & !flagP
//   (o, s)     orientation o = 0: P's frame is on the low lines, (a, b) = (p, q); o = 1: (a, b) = (q, p). For a split s,
//              min_side <= s <= L - min_side: first = #{l < s : a(l)}, last = #{l >= s : b(l)}; admissible iff 8 first >= 7 s and
//              8 last >= 7 (L - s) (the 7/8 tolerates the line the tear crosses and a few damaged ones; a rule constant)
//   candidate  some (o, s) is admissible; the tear is the admissible pair with the largest first + last, ties to the lower o, then the
//              lower s. Axis 2: axis 0's tear where it has one, else axis 1's. The record is {axis * 2 + o, s, first, last}, a capture that is
//              no candidate {-1, -1, 0, 0} (CIMBAR_HIP_TAP_ONCE_TEAR)
//   pass 1     list 1 = the representatives without the candidates, in capture order
//   guard      a candidate whose two neighbour runs' representatives both came back with full masks is TORN (role 3): never decoded,
//              mask 0, a zeroed slot, its run's row zero. Every other candidate joins list 2, in capture order, as a fallback.
//   R12 k_repeat_tear         one workgroup per capture, behind the walk: the record
//   R4t k_repeat_lists_tear   R4 without the candidates: list 1 is no longer "by run", so one wavefront compacts it and writes pos[run] =
//                             the representative's place in list 1 (-1: a candidate's run) and the call's words {|list 1|, 0}
//   R5t k_repeat_lists2_tear  R5 through pos, with the guard
//   R10t k_rescue_save_tear   R10 through pos (pass 1's scratch is by list position)
// Everything else of the call is the kernels above, unchanged: a torn capture's mask is 0 and its slot zero by R7, its run's row by R8.
constexpr int RT_LINE_DEFAULT = 750, RT_SIDE_DEFAULT = 2;
constexpr int RT_LSTRIDE = 128;                                            // STITCH_LMAX <= 128
enum { RP_ROLE_TORN = CIMBAR_HIP_ONCE_TORN };
enum { RTW_LEN1 = 0, RTW_LEN2 = 1, RT_WORDS = 2 };                         // a call's words with the setting on: |list 1|, |list 2| (the run count stays where the walk wrote it)

// R12: workgroup k. Integer arithmetic only. The per-line counts are LDS atomics: a dword of four cells lies on one grid row (one add of
// 0..4 per side), and on four consecutive grid columns (one add per equal cell).
__global__ __launch_bounds__(256) void k_repeat_tear(const uint8_t* __restrict__ sig, const int* __restrict__ runs, const int* __restrict__ rcount, int n,
                                                     const uint8_t* __restrict__ line_tab, int axis, int line_permille, int min_side,
                                                     int32_t* __restrict__ tap)
{
	const int k = blockIdx.x, t = threadIdx.x;
	bool eligible = k >= 1 && k + 1 < n;
	if (eligible) {
		const int r = runs[k];
		eligible = runs[k - 1] >= 0 && r >= 0 && runs[k + 1] >= 0 && rcount[r] == 1;
	}
	if (!eligible) {                                                     // (uniform over the workgroup)
		if (t < 4) tap[(size_t)k * 4 + t] = t < 2 ? -1 : 0;
		return;
	}
	__shared__ uint32_t s_cnt[2][2][RT_LSTRIDE];                         // [axis][P | N][line]
	__shared__ uint16_t s_pre[2][2][RT_LSTRIDE + 2];                     // [axis][p | q][s] = the flagged lines below s, s = 0 .. L
	__shared__ uint8_t s_pq[2][2][RT_LSTRIDE];
	__shared__ uint32_t s_best;
	for (int e = t; e < 2 * 2 * RT_LSTRIDE; e += 256) (&s_cnt[0][0][0])[e] = 0u;
	if (t == 0) s_best = 0u;
	__syncthreads();
	const bool ax0 = axis != 1, ax1 = axis != 0;
	constexpr int W = NCELLS / 4;
	const uint32_t* c = reinterpret_cast<const uint32_t*>(sig + (size_t)k * NCELLS);
	const uint32_t* row_tab = reinterpret_cast<const uint32_t*>(line_tab);
	const uint32_t* col_tab = reinterpret_cast<const uint32_t*>(line_tab + NCELLS);
	for (int w = t; w < W; w += 256) {
		const uint32_t me = c[w], x = me ^ c[w - W], y = me ^ c[w + W];
		const uint32_t eP[4] = {(x & 0xFFu) == 0u, (x & 0xFF00u) == 0u, (x & 0xFF0000u) == 0u, (x >> 24) == 0u};
		const uint32_t eN[4] = {(y & 0xFFu) == 0u, (y & 0xFF00u) == 0u, (y & 0xFF0000u) == 0u, (y >> 24) == 0u};
		if (ax0) {
			const int row = (int)(row_tab[w] & 0xFFu);
			const uint32_t cp = eP[0] + eP[1] + eP[2] + eP[3], cn = eN[0] + eN[1] + eN[2] + eN[3];
			if (cp) atomicAdd(&s_cnt[0][0][row], cp);
			if (cn) atomicAdd(&s_cnt[0][1][row], cn);
		}
		if (ax1) {
			const uint32_t cols = col_tab[w];
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int col = (int)((cols >> (8 * j)) & 0xFFu);
				if (eP[j]) atomicAdd(&s_cnt[1][0][col], 1u);
				if (eN[j]) atomicAdd(&s_cnt[1][1][col], 1u);
			}
		}
	}
	__syncthreads();
	{
		const int ax = t >> 7, l = t & 127;
		bool p = false, q = false;
		if (l < stitch_lines(ax)) {
			const uint32_t need = (uint32_t)line_permille * (uint32_t)stitch_width(ax, l);
			const bool fP = s_cnt[ax][0][l] * 1000u >= need, fN = s_cnt[ax][1][l] * 1000u >= need;
			p = fP && !fN;
			q = fN && !fP;
		}
		s_pq[ax][0][l] = p ? 1 : 0;
		s_pq[ax][1][l] = q ? 1 : 0;
	}
	__syncthreads();
	if (t < 4) {
		const int ax = t >> 1, which = t & 1, L = stitch_lines(ax);
		uint32_t acc = 0;
		for (int s = 0; s <= L; ++s) {
			s_pre[ax][which][s] = (uint16_t)acc;
			if (s < L) acc += s_pq[ax][which][s];
		}
	}
	__syncthreads();
	// first / last of (ax, o, s): o = 0 takes p below the split and q from it on, o = 1 the reverse
	auto sides = [&](int ax, int o, int s, int& first, int& last) {
		const int L = stitch_lines(ax);
		first = s_pre[ax][o][s];
		last = s_pre[ax][o ^ 1][L] - s_pre[ax][o ^ 1][s];
	};
	for (int e = t; e < 2 * 2 * (RT_LSTRIDE + 1); e += 256) {
		const int ax = e / (2 * (RT_LSTRIDE + 1)), o = (e / (RT_LSTRIDE + 1)) & 1, s = e % (RT_LSTRIDE + 1);
		const int L = stitch_lines(ax);
		if (!(ax == 0 ? ax0 : ax1) || s < min_side || s > L - min_side) continue;
		int first, last;
		sides(ax, o, s, first, last);
		if (8 * first >= 7 * s && 8 * last >= 7 * (L - s))
			atomicMax(&s_best, 1u << 24 | (uint32_t)(1 - ax) << 23 | (uint32_t)(first + last) << 9 | (uint32_t)(1 - o) << 8 | (uint32_t)(255 - s));
	}
	__syncthreads();
	if (t == 0) {
		const uint32_t best = s_best;
		int32_t* row = tap + (size_t)k * 4;
		if (!best) { row[0] = -1; row[1] = -1; row[2] = 0; row[3] = 0; }
		else {
			const int ax = 1 - (int)((best >> 23) & 1u), o = 1 - (int)((best >> 8) & 1u), s = 255 - (int)(best & 255u);
			int first, last;
			sides(ax, o, s, first, last);
			row[0] = ax * 2 + o; row[1] = s; row[2] = first; row[3] = last;
		}
	}
}

// R4t: one wavefront, 64 captures per step. A candidate (tap row k, word 0 >= 0: a run of one) takes RP_ROLE_TORN for now and stays off
// list 1; pos[r] = where run r's representative stands in list 1, -1 for a candidate's run.
__global__ __launch_bounds__(64) void k_repeat_lists_tear(const int* __restrict__ runs, const int* __restrict__ rmem, const int* __restrict__ rcount, int n,
                                                          const int32_t* __restrict__ tap, int* __restrict__ roles, int* __restrict__ list1,
                                                          int* __restrict__ pos, int* __restrict__ words)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull;
	int base = 0;
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		const int r = k < n ? runs[k] : -1;
		const bool rep = r >= 0 && repeat_rep(rmem, rcount, r) == k;
		const bool cand = rep && tap[(size_t)k * 4] >= 0;
		const bool take = rep && !cand;
		const unsigned long long tb = __ballot(take);
		if (k < n) roles[k] = r < 0 ? RP_ROLE_UNUSABLE : take ? RP_ROLE_REP : cand ? RP_ROLE_TORN : RP_ROLE_SKIPPED;
		if (take) {
			const int at = base + (int)__popcll(tb & below);
			list1[at] = k;
			pos[r] = at;
		}
		if (cand) pos[r] = -1;
		base += (int)__popcll(tb);
	}
	if (lane == 0) { words[RTW_LEN1] = base; words[RTW_LEN2] = 0; }
}

// R5t: as R5, with rep_masks by list position. A candidate is torn for good when the representatives of its two neighbours' runs both came
// back with full masks; otherwise it joins list 2 as a fallback, in capture order among the others (map as in R5).
__global__ __launch_bounds__(64) void k_repeat_lists2_tear(const int* __restrict__ runs, const uint32_t* __restrict__ rep_masks, const int* __restrict__ pos, int n,
                                                           int* __restrict__ roles, int* __restrict__ list2, int* __restrict__ count2, int* __restrict__ map)
{
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull;
	auto full = [&](int k) { const int at = pos[runs[k]]; return at >= 0 && (rep_masks[at] & RP_FULL) == RP_FULL; };
	int base = 0;
	for (int k0 = 0; k0 < n; k0 += 64) {
		const int k = k0 + lane;
		bool take = false;
		if (k < n) {
			const int role = roles[k];
			if (role == RP_ROLE_SKIPPED) take = !full(k);
			else if (role == RP_ROLE_TORN) take = !(full(k - 1) && full(k + 1));   // (a candidate has both neighbours, and both are in runs)
		}
		const unsigned long long tb = __ballot(take);
		if (take) {
			const int at = base + (int)__popcll(tb & below);
			roles[k] = RP_ROLE_FALLBACK;
			list2[at] = k;
			if (map) map[k] = at;
		}
		base += (int)__popcll(tb);
	}
	if (lane == 0) *count2 = base;
}

// R10t: R10 where run r's representative stands at pos[r] in pass 1's batch (a qualifying run has two members or more, so pos[r] >= 0).
// nruns may be any bound on the run count up to n: the member counts at and above it are zero (the host zeroes all n before the walk).
__global__ __launch_bounds__(256) void k_rescue_save_tear(const uint32_t* __restrict__ plane, const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors,
                                                          const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                          const uint32_t* __restrict__ rep_masks, const int* __restrict__ rmem, const int* __restrict__ rcount,
                                                          int nruns, CarryStore cs, int* __restrict__ slot_run, int* __restrict__ smem, int* __restrict__ map,
                                                          int* __restrict__ nslots, const int* __restrict__ pos)
{
	rescue_save_body<true>(plane, symbols, colors, drift, flood_flag, rep_masks, rmem, rcount, nruns, cs, slot_run, smem, map, nslots, pos);
}

// ------------------------------------------------------------------------------------------------ tear salvage (the plain once-calls, opt-in)
// cimbar_hip_set_once_tear_salvage, effective with the run rescue and tear skipping both on. A torn candidate beside an incomplete run is
// decoded whole in pass 2 and delivers next to nothing, yet on every line on that run's side of the tear its cells are cells of the run's
// frame. With the setting effective such a candidate joins the rescue's group decode of the run as a PARTIAL member:
//   sides      candidate k, record {w, s, first, last}, axis = w >> 1, o = w & 1, L lines, guard g: low = [0, s - g), high = [s + g, L); its
//              P side (towards capture k - 1) is low when o = 0, high when o = 1, its N side the other. An empty side gives no partial.
//   partials   run r (no candidate's run), members f .. e: the following partial is capture e + 1 with its P side, the preceding partial
//              capture f - 1 with its N side, each if that capture is a candidate with role FALLBACK
//   qualifies  the representative's mask is not full and the run has two members or a partial: at most min(|list 1|, 2 |list 2|) runs, as
//              each has its representative in list 1 and a member or an adjacent candidate in list 2, which serves two runs at most
//   order      the full members, the preceding partial, the following partial; a partial joins only while the row has fewer than GMAX members
//   tried      a qualifying run whose full members' masks, after pass 2, are together still not full
//   R10s k_rescue_save_salvage   R10t with that rule; the slot's row of `part` = {kp, axis_p, lo_p, hi_p, kf, axis_f, lo_f, hi_f}
//   R11s k_rescue_tried_salvage  gcount[slot] = the full members plus the partials of a tried run, gfull[slot] = the full members alone
//   G3p k_group_cells_salvage (combine.hip.inc) over gcount; k_rs LIVE and G4r k_group_end_rescue as they are, G4r over gfull: only the full
//   members' chunks and masks enter the row
constexpr int RV_GUARD_DEFAULT = 1, RV_GUARD_MAX = 16;

// a torn candidate k's side towards capture k - 1 (p_side) or towards k + 1 as a partial: {axis, lo, hi}. false: k is outside the call, is no
// candidate that pass 2 decodes, or the side is empty. tap: tear skipping's records; roles: as k_repeat_lists2_tear left them.
__device__ __forceinline__ bool salvage_side(const int32_t* __restrict__ tap, const int* __restrict__ roles, int k, int n, bool p_side, int guard, int& axis,
                                             int& lo, int& hi)
{
	axis = 0; lo = 0; hi = 0;
	if (k < 0 || k >= n || roles[k] != RP_ROLE_FALLBACK) return false;
	const int w = tap[(size_t)k * 4];
	if (w < 0) return false;                                             // (a fallback that is no candidate: a member of some run)
	const int s = tap[(size_t)k * 4 + 1], o = w & 1;
	axis = w >> 1;
	const bool low = p_side == (o == 0);
	lo = low ? 0 : s + guard;
	hi = low ? s - guard : stitch_lines(axis);
	return lo < hi;
}

__global__ __launch_bounds__(256) void k_rescue_save_salvage(const uint32_t* __restrict__ plane, const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors,
                                                             const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                             const uint32_t* __restrict__ rep_masks, const int* __restrict__ rmem, const int* __restrict__ rcount,
                                                             int nruns, CarryStore cs, int* __restrict__ slot_run, int* __restrict__ smem, int* __restrict__ map,
                                                             int* __restrict__ nslots, const int* __restrict__ pos, const int* __restrict__ roles,
                                                             const int32_t* __restrict__ tap, int n, int guard, int32_t* __restrict__ part)
{
	rescue_save_body<true, true>(plane, symbols, colors, drift, flood_flag, rep_masks, rmem, rcount, nruns, cs, slot_run, smem, map, nslots, pos, roles, tap, n, guard,
	                             part);
}

// R11s: R11 over the full members, with the second count
__global__ __launch_bounds__(256) void k_rescue_tried_salvage(const int* __restrict__ nslots, int slots, const int* __restrict__ slot_run, const int* __restrict__ smem,
                                                              const int* __restrict__ rcount, const uint32_t* __restrict__ masks, const int32_t* __restrict__ part,
                                                              int* __restrict__ gcount, int* __restrict__ gfull, uint32_t* __restrict__ gdisp)
{
	const int s = blockIdx.x * 256 + threadIdx.x;
	if (s >= slots) return;
	int m = 0, all_m = 0;
	if (s < *nslots) {
		const int cnt = rcount[slot_run[s]];
		uint32_t all = 0;
		for (int j = 0; j < cnt; ++j) all |= masks[smem[(size_t)s * GMAX + j]];
		m = (all & RP_FULL) != RP_FULL ? cnt : 0;
		all_m = m ? m + (part[(size_t)s * 8] >= 0 ? 1 : 0) + (part[(size_t)s * 8 + 4] >= 0 ? 1 : 0) : 0;
	}
	gcount[s] = all_m;
	gfull[s] = m;
	gdisp[s] = 0u;
}
