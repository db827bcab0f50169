// stitch.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace, after combine.hip.inc).
// S1-S2: torn-capture stitching -- a frame that two consecutive captures each show one side of, decoded from the cells of both
// ------------------------------------------------------------------------------------------------ the rule
// A rolling shutter that crosses a display refresh shows frame A on one side of a line and frame B on the other; the next capture shows B,
// then C. The two captures agree where both show B. A batch is decoded capture by capture first (enqueue(), unchanged). Then, for
// consecutive captures k and k+1 and the caller's axis:
//   lines      axis 0: line(i) = cell i's grid row (y_i - OFFSET) / PITCH, L = DIM_Y; axis 1: its grid column (x_i - OFFSET) / PITCH, L = DIM_X.
//              width(l) = the cells on line l (fewer on the lines that cross the anchors)
//   eq(i)      symbol AND colour equal, with agreeing_cells' masks (combine.hip.inc)
//   cnt(l)     = the sum of eq over line l; flag(l) = cnt(l) * 1000 >= min_agree_permille * width(l)   (min_agree_permille <= 0: 750)
//   band       a = the lowest flagged line, b = the highest flagged line + 1, f = the flagged lines
//   candidate  both captures usable, f >= 1, b - a >= min_band (min_band <= 0: 2), 4 f >= 3 (b - a) (a few damaged lines inside the band
//              are tolerated), and a > 0 or b < L (a band over the whole frame is two captures of one frame: the group decode's case)
//   split      s = (a + b) >> 1, the line farthest from both tears. Direction 0: cell i comes from capture k+1 if line(i) < s, else from
//              capture k (the later capture's low lines and the earlier one's high lines show the shared frame); direction 1 is the
//              reverse, for a sensor read the other way round. Symbol and colour are the chosen capture's own decisions.
//   decode     slot 2k + d holds pair k, direction d. A candidate's two cell sets go through k_rs<.., LIVE> and the aligned_stream
//              bookkeeping of one frame (group_end_body's cmask; modes 4 / 8: the coupled stream). No colour-correction matrix is
//              derived, read or carried; nothing is filled in from the members (they show other frames); no vote; an erasure retry only with
//              cimbar_hip_set_stitch_erasure on (S3 / S4 at the end of this file).
//              smask = that decode's own mask; slots of chunks outside it are zero.
// The wrong direction yields chunks of a neighbouring frame or nothing: every chunk in a mask is a genuine chunk, and a sink dedups.
//   S1 k_stitch_pairs  one workgroup per pair: cnt, the tear record {a, b, s, f}, the two slots' live flags and, for a candidate, both
//                      directions' stitched symbols and colours
//   K3 k_rs            over 2 (n - 1) slots (LIVE: the workgroups past the last candidate and the wavefronts of a non-candidate return at once)
//   S2 k_stitch_end    one workgroup per slot: the aligner walk, the mask, zeroes for undelivered chunks; all zeroes for a non-live slot
// ------------------------------------------------------------------------------------------------ the stream calls
// cimbar_hip_decode_batch_stitched_stream / _scan_extract_decode_batch_stitched_stream_fmt: a call of n captures reports n rows, row 0 = (the last
// capture of the stream call before, capture 0), row r = (capture r - 1, capture r); row r, direction d is slot 2r + d. A pair closes with its
// second capture, so the carry is always one capture's decided cells and a word saying whether that capture is usable; nothing is ever open.
// Row 0 without a usable carry (after create / reset, or a carried capture whose extraction failed) is a non-candidate {-1, -1, -1, 0} with
// zero counts. Everything else is the rule above, through the same body: k_stitch_pairs_stream is its CARRY instance, K3 and S2 run over 2n slots.
// ------------------------------------------------------------------------------------------------ strips (cimbar_hip_set_stitch_strips, S in 2..8)
// A tear is a straight line of the sensor, so roll and perspective put it on a slant in the deskewed frame: with the two tears closer than
// 3/4 of the slant's rise no whole line reaches 750, though every column still has its clean shared lines. The frame is cut across the
// lines into S strips and the band is found strip by strip:
//   strip      across(i) = the cell's index on the other axis (axis 0: its grid column, A = DIM_X; axis 1: its grid row, A = DIM_Y);
//              strip(i) = across(i) * S / A. width(l, j) = the cells of line l in strip j (> 0 for S <= 8 in every mode: build_tables checks)
//   flag(l, j) cnt(l, j) * 1000 >= min_agree_permille * width(l, j), cnt(l, j) = the sum of eq over those cells
//   located    a_j, b_j, f_j as a, b, f above, of strip j's flags; located iff f_j >= 1, b_j - a_j >= min_band and 4 f_j >= 3 (b_j - a_j)
//   candidate  both captures usable, 2 * located >= S, and some located strip with a_j > 0 or b_j < L
//   splits     a located strip: s_j = (a_j + b_j) >> 1; any other takes the split of the nearest located strip by index, the lower one on a tie.
//              Cell i is chosen as above with s_{strip(i)} for s.
//   record     {min a_j, max b_j over the located strips, s_{S >> 1}, the sum of f_j}; a non-candidate {-1, -1, -1, the sum of f_j}
// Slots, the Reed-Solomon pass, S2 and *n_slots are the ones above. S = 1 is k_stitch_pairs / k_stitch_pairs_stream themselves.
//   S1 k_stitch_pairs_strips / k_stitch_pairs_strips_stream  the same workgroup per pair with cnt [8][128] in LDS; also the per-strip records
//                      {a_j, b_j, s_j, f_j} and cnt(l, j) for the taps (lines stays cnt(l), the sum over the strips)
constexpr int STITCH_AGREE_DEFAULT = 750, STITCH_BAND_DEFAULT = 2;
constexpr int STITCH_LMAX = DIM_X > DIM_Y ? DIM_X : DIM_Y;
static_assert(STITCH_LMAX <= 128, "the line flags fit two ballots");
static_assert(TOP_W % 4 == 0 && DIM_X % 4 == 0 && TOP_CELLS % 4 == 0 && MID_CELLS % 4 == 0, "axis 0: every dword of cells lies on one grid row");

__device__ __host__ constexpr int stitch_lines(int axis) { return axis == 0 ? DIM_Y : DIM_X; }
__device__ __forceinline__ int stitch_width(int axis, int l)
{
	if (axis == 0) return (l < MARKER || l >= DIM_Y - MARKER) ? TOP_W : DIM_X;
	return (l < MARKER || l >= DIM_X - MARKER) ? DIM_Y - 2 * MARKER : DIM_Y;
}

// S1. line_tab: [2][NCELLS] u8, the grid row and the grid column of every cell. status == nullptr: every capture usable, else the capture
// path's extraction status, stride ints apart (> 0: usable). tears [rows][4], lines [rows][L] u16, live / ssym / scol per slot;
// *n_slots (zeroed by the host) = the slots up to the last candidate's, for the Reed-Solomon launches: a batch without a candidate costs
// them nothing but the launch. A non-candidate writes its record and cleared flags only.
// The stream calls' carry (cimbar_hip_decode_batch_stitched_stream): the last capture of the stream call before, two slots used in turn. A call
// reads slot `cur` and writes the other one, so the writer needs no place behind the readers; the host flips `cur` with every call.
constexpr int SS_CELLS = (NCELLS + 15) & ~15;   // slot stride, bytes
struct StitchCarry {
	uint8_t* symbols; uint8_t* colors;   // [2][SS_CELLS]
	uint32_t* usable;                    // [2] != 0: the slot holds a usable capture (0 after create / reset and for a capture whose extraction failed)
	int cur;                             // the slot this call reads
};

// CARRY = false: workgroup k of n - 1 is the pair (capture k, capture k + 1). CARRY = true: workgroup r of n is the row (capture r - 1,
// capture r), the carried capture for r = 0; the last row's workgroup leaves capture n - 1 as the next call's carry.
template <bool CARRY>
__device__ __forceinline__ void stitch_pairs_body(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                  const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab, int axis,
                                                  int min_agree, int min_band, int32_t* __restrict__ tears, uint16_t* __restrict__ lines,
                                                  uint32_t* __restrict__ live, int* __restrict__ n_slots, uint8_t* __restrict__ ssym,
                                                  uint8_t* __restrict__ scol, const StitchCarry cy)
{
	const int k = blockIdx.x;
	constexpr int W = NCELLS / 4;
	constexpr uint32_t CM = 0x01010101u * (uint32_t)(NCOLORS - 1);
	const int L = stitch_lines(axis);
	const uint32_t *s0, *c0, *s1, *c1;
	[[maybe_unused]] bool pair_usable = true;
	if constexpr (CARRY) {
		if (k >= n) return;
		s1 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
		c1 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
		const bool later_usable = !status || status[(size_t)k * stride] > 0;
		if (k == n - 1) {   // the next call's carry, into the slot nobody reads in this call
			uint32_t* ns = reinterpret_cast<uint32_t*>(cy.symbols + (size_t)(cy.cur ^ 1) * SS_CELLS);
			uint32_t* nc = reinterpret_cast<uint32_t*>(cy.colors + (size_t)(cy.cur ^ 1) * SS_CELLS);
			for (int w = threadIdx.x; w < W; w += 256) { ns[w] = s1[w]; nc[w] = c1[w]; }
			if (threadIdx.x == 0) cy.usable[cy.cur ^ 1] = later_usable ? 1u : 0u;
		}
		if (k == 0) {
			if (!cy.usable[cy.cur]) {   // nothing carried, or a capture whose extraction failed: a non-candidate without counts
				if (threadIdx.x < L) lines[threadIdx.x] = 0;
				if (threadIdx.x == 0) {
					tears[0] = tears[1] = tears[2] = -1; tears[3] = 0;
					live[0] = live[1] = 0u;
				}
				return;
			}
			s0 = reinterpret_cast<const uint32_t*>(cy.symbols + (size_t)cy.cur * SS_CELLS);
			c0 = reinterpret_cast<const uint32_t*>(cy.colors + (size_t)cy.cur * SS_CELLS);
			pair_usable = later_usable;
		} else {
			s0 = s1 - W; c0 = c1 - W;
			pair_usable = later_usable && (!status || status[(size_t)(k - 1) * stride] > 0);
		}
	} else {
		if (k + 1 >= n) return;
		s0 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
		c0 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
		s1 = s0 + W; c1 = c0 + W;
	}
	__shared__ uint32_t s_cnt[128];
	__shared__ int s_split;
	if (threadIdx.x < 128) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t* lt = reinterpret_cast<const uint32_t*>(line_tab + (size_t)axis * NCELLS);
	for (int w = threadIdx.x; w < W; w += 256) {
		const uint32_t x = ((s0[w] ^ s1[w]) & 0x0F0F0F0Fu) | ((c0[w] ^ c1[w]) & CM);
		const uint32_t ids = lt[w];
		const uint32_t e0 = (x & 0xFFu) == 0u, e1 = (x & 0xFF00u) == 0u, e2 = (x & 0xFF0000u) == 0u, e3 = (x >> 24) == 0u;
		if (ids == (ids & 0xFFu) * 0x01010101u) {   // (axis 0: always)
			const uint32_t c = e0 + e1 + e2 + e3;
			if (c) atomicAdd(&s_cnt[ids & 0xFFu], c);
		} else {
			if (e0) atomicAdd(&s_cnt[ids & 0xFFu], 1u);
			if (e1) atomicAdd(&s_cnt[(ids >> 8) & 0xFFu], 1u);
			if (e2) atomicAdd(&s_cnt[(ids >> 16) & 0xFFu], 1u);
			if (e3) atomicAdd(&s_cnt[ids >> 24], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 64) {
		const int lane = threadIdx.x;
		bool usable;
		if constexpr (CARRY) usable = pair_usable;
		else usable = !status || (status[(size_t)k * stride] > 0 && status[(size_t)(k + 1) * stride] > 0);
		bool fl[2];
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const int l = lane + 64 * h;
			const uint32_t c = l < L ? s_cnt[l] : 0u;
			fl[h] = l < L && (unsigned long long)c * 1000ull >= (unsigned long long)min_agree * (unsigned long long)stitch_width(axis, l < L ? l : 0);
			if (l < L) lines[(size_t)k * L + l] = (uint16_t)c;
		}
		const unsigned long long lo = __ballot(fl[0]), hi = __ballot(fl[1]);
		if (lane == 0) {
			const int f = (int)__popcll(lo) + (int)__popcll(hi);
			int a = -1, b = -1, s = -1;
			if (f >= 1) {
				const int lowest = lo ? __ffsll((long long)lo) - 1 : 64 + __ffsll((long long)hi) - 1;
				const int highest = hi ? 127 - __clzll((long long)hi) : 63 - __clzll((long long)lo);
				const int bb = highest + 1;
				if (usable && bb - lowest >= min_band && 4 * f >= 3 * (bb - lowest) && (lowest > 0 || bb < L)) { a = lowest; b = bb; s = (a + b) >> 1; }
			}
			int32_t* t = tears + (size_t)k * 4;
			t[0] = a; t[1] = b; t[2] = s; t[3] = f;
			live[2 * k] = live[2 * k + 1] = a >= 0 ? 1u : 0u;
			if (a >= 0) atomicMax(n_slots, 2 * k + 2);
			s_split = s;
		}
	}
	__syncthreads();
	const int s = s_split;
	if (s < 0) return;
	uint32_t* os0 = reinterpret_cast<uint32_t*>(ssym + (size_t)(2 * k) * NCELLS);
	uint32_t* oc0 = reinterpret_cast<uint32_t*>(scol + (size_t)(2 * k) * NCELLS);
	uint32_t *os1 = os0 + W, *oc1 = oc0 + W;
	for (int w = threadIdx.x; w < W; w += 256) {
		const uint32_t ids = lt[w];
		// bytes whose line lies below the split: direction 0 takes them from capture k + 1, direction 1 from capture k
		const uint32_t m = ((int)(ids & 0xFFu) < s ? 0xFFu : 0u) | ((int)((ids >> 8) & 0xFFu) < s ? 0xFF00u : 0u) |
		                   ((int)((ids >> 16) & 0xFFu) < s ? 0xFF0000u : 0u) | ((int)(ids >> 24) < s ? 0xFF000000u : 0u);
		const uint32_t a0 = s0[w], a1 = s1[w], b0 = c0[w], b1 = c1[w];
		os0[w] = (a1 & m) | (a0 & ~m);
		os1[w] = (a0 & m) | (a1 & ~m);
		oc0[w] = (b1 & m) | (b0 & ~m);
		oc1[w] = (b0 & m) | (b1 & ~m);
	}
}

__global__ __launch_bounds__(256) void k_stitch_pairs(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                      const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab, int axis,
                                                      int min_agree, int min_band, int32_t* __restrict__ tears, uint16_t* __restrict__ lines,
                                                      uint32_t* __restrict__ live, int* __restrict__ n_slots, uint8_t* __restrict__ ssym,
                                                      uint8_t* __restrict__ scol)
{
	stitch_pairs_body<false>(symbols, colors, n, status, stride, line_tab, axis, min_agree, min_band, tears, lines, live, n_slots, ssym, scol, StitchCarry{});
}

__global__ __launch_bounds__(256) void k_stitch_pairs_stream(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                             const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab, int axis,
                                                             int min_agree, int min_band, int32_t* __restrict__ tears, uint16_t* __restrict__ lines,
                                                             uint32_t* __restrict__ live, int* __restrict__ n_slots, uint8_t* __restrict__ ssym,
                                                             uint8_t* __restrict__ scol, const StitchCarry cy)
{
	stitch_pairs_body<true>(symbols, colors, n, status, stride, line_tab, axis, min_agree, min_band, tears, lines, live, n_slots, ssym, scol, cy);
}

// S1 with strips. strip_width: [STITCH_SMAX][128] u16, width(l, j) of the call's axis and S (build_tables). strips [rows][S][4]
// {a_j, b_j, s_j, f_j}: a_j = b_j = -1 for a strip that is not located, s_j = its resolved split, -1 in a non-candidate;
// strip_lines [rows][S][L] u16. Everything else as stitch_pairs_body, whose operand selection and carry hand-over this repeats.
constexpr int STITCH_SMAX = 8;
__device__ __forceinline__ uint32_t stitch_strip(int axis, uint32_t across, uint32_t S) 
{
	return axis == 0 ? across * S / (uint32_t)DIM_X : across * S / (uint32_t)DIM_Y;   // (divisions by constants)
}

template <bool CARRY>
__device__ __forceinline__ void stitch_pairs_strips_body(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                         const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab,
                                                         const uint16_t* __restrict__ strip_width, int axis, int S, int min_agree, int min_band,
                                                         int32_t* __restrict__ tears, uint16_t* __restrict__ lines, int32_t* __restrict__ strips,
                                                         uint16_t* __restrict__ strip_lines, uint32_t* __restrict__ live, int* __restrict__ n_slots,
                                                         uint8_t* __restrict__ ssym, uint8_t* __restrict__ scol, const StitchCarry cy)
{
	const int k = blockIdx.x;
	constexpr int W = NCELLS / 4;
	constexpr uint32_t CM = 0x01010101u * (uint32_t)(NCOLORS - 1);
	const int L = stitch_lines(axis);
	const uint32_t *s0, *c0, *s1, *c1;
	bool usable;
	if constexpr (CARRY) {
		if (k >= n) return;
		s1 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
		c1 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
		const bool later_usable = !status || status[(size_t)k * stride] > 0;
		if (k == n - 1) {   // the next call's carry, into the slot nobody reads in this call
			uint32_t* ns = reinterpret_cast<uint32_t*>(cy.symbols + (size_t)(cy.cur ^ 1) * SS_CELLS);
			uint32_t* nc = reinterpret_cast<uint32_t*>(cy.colors + (size_t)(cy.cur ^ 1) * SS_CELLS);
			for (int w = threadIdx.x; w < W; w += 256) { ns[w] = s1[w]; nc[w] = c1[w]; }
			if (threadIdx.x == 0) cy.usable[cy.cur ^ 1] = later_usable ? 1u : 0u;
		}
		if (k == 0) {
			if (!cy.usable[cy.cur]) {   // nothing carried, or a capture whose extraction failed: a non-candidate without counts
				if (threadIdx.x < L) lines[threadIdx.x] = 0;
				for (int e = threadIdx.x; e < S * L; e += 256) strip_lines[e] = 0;
				if (threadIdx.x < S) {
					int32_t* r = strips + (size_t)threadIdx.x * 4;
					r[0] = r[1] = r[2] = -1; r[3] = 0;
				}
				if (threadIdx.x == 0) {
					tears[0] = tears[1] = tears[2] = -1; tears[3] = 0;
					live[0] = live[1] = 0u;
				}
				return;
			}
			s0 = reinterpret_cast<const uint32_t*>(cy.symbols + (size_t)cy.cur * SS_CELLS);
			c0 = reinterpret_cast<const uint32_t*>(cy.colors + (size_t)cy.cur * SS_CELLS);
			usable = later_usable;
		} else {
			s0 = s1 - W; c0 = c1 - W;
			usable = later_usable && (!status || status[(size_t)(k - 1) * stride] > 0);
		}
	} else {
		if (k + 1 >= n) return;
		s0 = reinterpret_cast<const uint32_t*>(symbols + (size_t)k * NCELLS);
		c0 = reinterpret_cast<const uint32_t*>(colors + (size_t)k * NCELLS);
		s1 = s0 + W; c1 = c0 + W;
		usable = !status || (status[(size_t)k * stride] > 0 && status[(size_t)(k + 1) * stride] > 0);
	}
	__shared__ uint32_t s_cnt[STITCH_SMAX * 128];   // [strip][line]
	__shared__ int s_a[STITCH_SMAX], s_b[STITCH_SMAX], s_f[STITCH_SMAX], s_split[STITCH_SMAX];
	__shared__ int s_cand;
	for (int e = threadIdx.x; e < STITCH_SMAX * 128; e += 256) s_cnt[e] = 0;
	__syncthreads();
	const uint32_t* lt = reinterpret_cast<const uint32_t*>(line_tab + (size_t)axis * NCELLS);
	const uint32_t* at = reinterpret_cast<const uint32_t*>(line_tab + (size_t)(axis ^ 1) * NCELLS);   // the other axis' row: across(i)
	const uint32_t uS = (uint32_t)S;
	for (int w = threadIdx.x; w < W; w += 256) {
		const uint32_t x = ((s0[w] ^ s1[w]) & 0x0F0F0F0Fu) | ((c0[w] ^ c1[w]) & CM);
		const uint32_t ids = lt[w], ac = at[w];
		const uint32_t e0 = (x & 0xFFu) == 0u, e1 = (x & 0xFF00u) == 0u, e2 = (x & 0xFF0000u) == 0u, e3 = (x >> 24) == 0u;
		const uint32_t j0 = stitch_strip(axis, ac & 0xFFu, uS), j1 = stitch_strip(axis, (ac >> 8) & 0xFFu, uS);
		const uint32_t j2 = stitch_strip(axis, (ac >> 16) & 0xFFu, uS), j3 = stitch_strip(axis, ac >> 24, uS);
		if (ids == (ids & 0xFFu) * 0x01010101u && j0 == j1 && j0 == j2 && j0 == j3) {   // the four cells share line and strip
			const uint32_t c = e0 + e1 + e2 + e3;
			if (c) atomicAdd(&s_cnt[j0 * 128u + (ids & 0xFFu)], c);
		} else {
			if (e0) atomicAdd(&s_cnt[j0 * 128u + (ids & 0xFFu)], 1u);
			if (e1) atomicAdd(&s_cnt[j1 * 128u + ((ids >> 8) & 0xFFu)], 1u);
			if (e2) atomicAdd(&s_cnt[j2 * 128u + ((ids >> 16) & 0xFFu)], 1u);
			if (e3) atomicAdd(&s_cnt[j3 * 128u + (ids >> 24)], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 64) {
		const int lane = threadIdx.x;
		uint32_t tot[2] = {0u, 0u};
		for (int j = 0; j < S; ++j) {   // (S is the same in every lane: the ballots see the whole wavefront)
			bool fl[2];
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const int l = lane + 64 * h;
				const uint32_t c = l < L ? s_cnt[j * 128 + l] : 0u;
				const uint32_t wd = l < L ? strip_width[j * 128 + l] : 0u;
				fl[h] = l < L && (unsigned long long)c * 1000ull >= (unsigned long long)min_agree * (unsigned long long)wd;
				if (l < L) strip_lines[((size_t)k * S + j) * L + l] = (uint16_t)c;
				tot[h] += c;
			}
			const unsigned long long lo = __ballot(fl[0]), hi = __ballot(fl[1]);
			if (lane == 0) {
				const int f = (int)__popcll(lo) + (int)__popcll(hi);
				int a = -1, b = -1;
				if (f >= 1) {
					const int lowest = lo ? __ffsll((long long)lo) - 1 : 64 + __ffsll((long long)hi) - 1;
					const int highest = hi ? 127 - __clzll((long long)hi) : 63 - __clzll((long long)lo);
					const int bb = highest + 1;
					if (bb - lowest >= min_band && 4 * f >= 3 * (bb - lowest)) { a = lowest; b = bb; }
				}
				s_a[j] = a; s_b[j] = b; s_f[j] = f;
			}
		}
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const int l = lane + 64 * h;
			if (l < L) lines[(size_t)k * L + l] = (uint16_t)tot[h];
		}
		if (lane == 0) {
			int located = 0, fsum = 0, amin = L, bmax = 0;
			bool partial = false;
			for (int j = 0; j < S; ++j) {
				fsum += s_f[j];
				if (s_a[j] < 0) continue;
				++located;
				amin = min(amin, s_a[j]); bmax = max(bmax, s_b[j]);
				partial = partial || s_a[j] > 0 || s_b[j] < L;
			}
			const bool cand = usable && 2 * located >= S && partial;
			for (int j = 0; j < S; ++j) {
				int sj = -1;
				if (cand) {
					int from = j;   // the nearest located strip by index, the lower one on a tie
					for (int d = 0; d < S; ++d) {
						if (j - d >= 0 && s_a[j - d] >= 0) { from = j - d; break; }
						if (j + d < S && s_a[j + d] >= 0) { from = j + d; break; }
					}
					sj = (s_a[from] + s_b[from]) >> 1;
				}
				s_split[j] = sj;
				int32_t* r = strips + ((size_t)k * S + j) * 4;
				r[0] = s_a[j]; r[1] = s_b[j]; r[2] = sj; r[3] = s_f[j];
			}
			int32_t* t = tears + (size_t)k * 4;
			t[0] = cand ? amin : -1; t[1] = cand ? bmax : -1; t[2] = cand ? s_split[S >> 1] : -1; t[3] = fsum;
			live[2 * k] = live[2 * k + 1] = cand ? 1u : 0u;
			if (cand) atomicMax(n_slots, 2 * k + 2);
			s_cand = cand ? 1 : 0;
		}
	}
	__syncthreads();
	if (!s_cand) return;
	uint32_t* os0 = reinterpret_cast<uint32_t*>(ssym + (size_t)(2 * k) * NCELLS);
	uint32_t* oc0 = reinterpret_cast<uint32_t*>(scol + (size_t)(2 * k) * NCELLS);
	uint32_t *os1 = os0 + W, *oc1 = oc0 + W;
	for (int w = threadIdx.x; w < W; w += 256) {
		const uint32_t ids = lt[w], ac = at[w];
		// bytes whose line lies below their strip's split: direction 0 takes them from capture k + 1, direction 1 from capture k
		const uint32_t m = ((int)(ids & 0xFFu) < s_split[stitch_strip(axis, ac & 0xFFu, uS)] ? 0xFFu : 0u) |
		                   ((int)((ids >> 8) & 0xFFu) < s_split[stitch_strip(axis, (ac >> 8) & 0xFFu, uS)] ? 0xFF00u : 0u) |
		                   ((int)((ids >> 16) & 0xFFu) < s_split[stitch_strip(axis, (ac >> 16) & 0xFFu, uS)] ? 0xFF0000u : 0u) |
		                   ((int)(ids >> 24) < s_split[stitch_strip(axis, ac >> 24, uS)] ? 0xFF000000u : 0u);
		const uint32_t a0 = s0[w], a1 = s1[w], b0 = c0[w], b1 = c1[w];
		os0[w] = (a1 & m) | (a0 & ~m);
		os1[w] = (a0 & m) | (a1 & ~m);
		oc0[w] = (b1 & m) | (b0 & ~m);
		oc1[w] = (b0 & m) | (b1 & ~m);
	}
}

__global__ __launch_bounds__(256) void k_stitch_pairs_strips(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                             const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab,
                                                             const uint16_t* __restrict__ strip_width, int axis, int S, int min_agree, int min_band,
                                                             int32_t* __restrict__ tears, uint16_t* __restrict__ lines, int32_t* __restrict__ strips,
                                                             uint16_t* __restrict__ strip_lines, uint32_t* __restrict__ live, int* __restrict__ n_slots,
                                                             uint8_t* __restrict__ ssym, uint8_t* __restrict__ scol)
{
	stitch_pairs_strips_body<false>(symbols, colors, n, status, stride, line_tab, strip_width, axis, S, min_agree, min_band, tears, lines, strips,
	                                strip_lines, live, n_slots, ssym, scol, StitchCarry{});
}

__global__ __launch_bounds__(256) void k_stitch_pairs_strips_stream(const uint8_t* __restrict__ symbols, const uint8_t* __restrict__ colors, int n,
                                                                    const int* __restrict__ status, int stride, const uint8_t* __restrict__ line_tab,
                                                                    const uint16_t* __restrict__ strip_width, int axis, int S, int min_agree,
                                                                    int min_band, int32_t* __restrict__ tears, uint16_t* __restrict__ lines,
                                                                    int32_t* __restrict__ strips, uint16_t* __restrict__ strip_lines,
                                                                    uint32_t* __restrict__ live, int* __restrict__ n_slots, uint8_t* __restrict__ ssym,
                                                                    uint8_t* __restrict__ scol, const StitchCarry cy)
{
	stitch_pairs_strips_body<true>(symbols, colors, n, status, stride, line_tab, strip_width, axis, S, min_agree, min_band, tears, lines, strips,
	                               strip_lines, live, n_slots, ssym, scol, cy);
}

// S2: slot blockIdx.x of 2 (n - 1). Live: the aligned_stream bookkeeping over the slot's block flags, the symbol blocks then the colour
// blocks with one state (group_end_body's cmask); smask = that mask, chunks outside it are zeroed. Not live: zero chunks, mask 0.
__global__ __launch_bounds__(256) void k_stitch_end(const uint32_t* __restrict__ live, const uint8_t* __restrict__ rs_ok, uint8_t* __restrict__ schunks,
                                                    uint32_t* __restrict__ smasks)
{
	const int g = blockIdx.x;
	uint8_t* gc = schunks + (size_t)g * FRAME_BYTES;
	if (!live[g]) {
		for (int k = threadIdx.x; k < FRAME_BYTES; k += 256) gc[k] = 0;
		if (threadIdx.x == 0) smasks[g] = 0;
		return;
	}
	constexpr uint32_t FULL = (1u << CHUNKS) - 1u;
	__shared__ uint32_t s_mask;
	if (threadIdx.x < 64) {
		const int lane = threadIdx.x;
		const uint8_t* ok = rs_ok + (size_t)g * ALL_BLOCKS;
		static_assert(ALL_BLOCKS <= 128, "block flags fit two ballots");
		const unsigned long long lo = __ballot(lane < ALL_BLOCKS && ok[lane < ALL_BLOCKS ? lane : 0] != 0);
		const unsigned long long hi = ALL_BLOCKS > 64 ? __ballot(64 + lane < ALL_BLOCKS && ok[64 + lane < ALL_BLOCKS ? 64 + lane : 0] != 0) : 0ull;
		if (lane == 0) {
			FrameState st = {0, 0, 0, 0};
			uint8_t hdr[6] = {0, 0, 0, 0, 0, 0};
			unsigned radio = 0;
			for (int b = 0; b < ALL_BLOCKS; ++b) aligner_block(st, b, (int)(((b < 64 ? lo : hi) >> (b & 63)) & 1ull), nullptr, false, hdr, radio);
			s_mask = st.mask & FULL;
		}
	}
	__syncthreads();
	const uint32_t mask = s_mask;
	for (int j = 0; j < CHUNKS; ++j) {
		if (mask & (1u << j)) continue;
		uint8_t* dst = gc + (size_t)j * CHUNK;
		for (int k = threadIdx.x; k < CHUNK; k += 256) dst[k] = 0;
	}
	if (threadIdx.x == 0) smasks[g] = mask;
}

// ------------------------------------------------------------------------------------------------ erasure retry (cimbar_hip_set_stitch_erasure)
// Opt-in, plain stitched calls only (the stream calls carry cells, not planes or means), modes 68 / 67 / 66, behind S2 on the same stream:
// the retries of erasure.hip.inc over a slot's stitched cells, each cell's confidence taken in the capture the cell came from.
//   src(i)     the capture S1 took cell i of slot 2k + d from: k + 1 if (line(i) < s) != (d == 1), else k; s = the tear record's split, with
//              strips above 1 the resolved split s_j of strip(i) (read back from d_stears / d_sstrips: S1's own decision, not a second one)
//   d_sym(i)   k_erasure_frame's distance in capture src(i): popcount(the 8x8 hash of that capture's plane at the cell's final position ^ the
//              tile hash of the STITCHED symbol); final position = grid position + that capture's drift where it took a flood pass
//   margin(i)  k_colour_erasure_frame's margin in capture src(i): color_fit<true> on that capture's K1 cell mean, or on mean6x6 at its drifted
//              position where it took a flood pass, under that capture's ccm_used row (active flag included)
//   S3 k_stitch_erasure         a live slot whose smask lacks symbol chunks: d_sym of every cell into sdist[slot], then er_retry_blocks over
//                               the missing symbol chunks (score = max over a byte's two cells of d_sym - t_sym + 1) and er_commit
//   S4 k_stitch_colour_erasure  the same for the colour chunks, behind S3: margins into smargin[slot], score = c_margin - margin, max over a
//                               byte's four cells. A kernel of its own: er_retry_blocks may be called once per kernel.
// A slot that is not live, or lacks nothing, returns at its first test with worked[slot] = 0. Chunks already in smask, d_srs_ok, the tear
// records, the line counts, the stitched cells, the per-capture outputs and the carried matrix are not touched.
__device__ __forceinline__ int stitch_src(const uint8_t* __restrict__ line_tab, int axis, int S, const int32_t* __restrict__ tears,
                                          const int32_t* __restrict__ strips, int k, int d, int i)
{
	const int line = line_tab[(size_t)axis * NCELLS + i];
	int s;
	if (S > 1) {
		const uint32_t j = stitch_strip(axis, line_tab[(size_t)(axis ^ 1) * NCELLS + i], (uint32_t)S);
		s = strips[((size_t)k * S + j) * 4 + 2];
	} else s = tears[(size_t)k * 4 + 2];
	return ((line < s) != (d == 1)) ? k + 1 : k;
}

__global__ __launch_bounds__(256) void k_stitch_erasure(const uint32_t* __restrict__ plane, Tables tb, const int8_t* __restrict__ drift,
                                                        const uint32_t* __restrict__ flood_flag, const uint8_t* __restrict__ line_tab, int axis, int S,
                                                        const int32_t* __restrict__ tears, const int32_t* __restrict__ strips,
                                                        const uint32_t* __restrict__ live, const uint8_t* __restrict__ ssym,
                                                        const uint8_t* __restrict__ rs_ok, uint8_t* __restrict__ schunks, uint32_t* __restrict__ smasks,
                                                        uint8_t* sdist, uint32_t* __restrict__ worked, int t_sym, int e_max)
{
	if constexpr (LEGACY) return;                          // (one coupled stream: the setter refuses these modes; the host never launches it there)
	constexpr uint32_t SYM_MASK = (1u << SYM_CHUNKS) - 1u;
	const int g = blockIdx.x, k = g >> 1, d = g & 1;
	const uint32_t mask = live[g] ? smasks[g] : SYM_MASK;
	if ((mask & SYM_MASK) == SYM_MASK) {                   // (uniform over the workgroup)
		if (threadIdx.x == 0) worked[g] = 0;
		return;
	}
	const uint8_t* sym = ssym + (size_t)g * NCELLS;
	uint8_t* ds = sdist + (size_t)g * NCELLS;
	for (int i = threadIdx.x; i < NCELLS; i += 256) {
		const int f = stitch_src(line_tab, axis, S, tears, strips, k, d, i);
		const bool flooded = flood_flag[f] != 0;
		const ushort2 xy = tb.cell_xy[i];
		const int dx = flooded ? drift[((size_t)f * NCELLS + i) * 2] : 0, dy = flooded ? drift[((size_t)f * NCELLS + i) * 2 + 1] : 0;
		uint32_t rows[10];
		window_rows(plane + (size_t)f * PLANE_WORDS, (int)xy.x + dx - 1, (int)xy.y + dy - 1, rows);
		ds[i] = (uint8_t)__popcll(window_hash(rows, 4) ^ c_tile[sym[i] & 15u]);
	}
	if (threadIdx.x == 0) worked[g] = 1;
	__syncthreads();                                       // (the distances are read back below by other lanes of this workgroup)
	uint8_t* fc = schunks + (size_t)g * FRAME_BYTES;
	const uint32_t done = er_retry_blocks<int16_t, 0, SYM_BLOCKS>(SYM_MASK & ~mask, rs_ok + (size_t)g * ALL_BLOCKS, e_max, fc, [&](int b, int kb, bool ok) {
		const int sidx = (RS_BLOCK * b + kb) * 2;
		int best = -32768;
		uint32_t v = 0;
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			const int cell = tb.stream_cell[sidx + q];
			v = (v << 4) | (sym[cell] & 15u);
			if (!ok) {
				const int sc = (int)ds[cell] - t_sym + 1;
				best = sc > best ? sc : best;
			}
		}
		return ErByte{v, best};
	});
	er_commit(mask | done, smasks + g, fc, 0, SYM_CHUNKS);
}

__global__ __launch_bounds__(256) void k_stitch_colour_erasure(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                               const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                               const float* __restrict__ ccm_used, const uint8_t* __restrict__ line_tab, int axis, int S,
                                                               const int32_t* __restrict__ tears, const int32_t* __restrict__ strips,
                                                               const uint32_t* __restrict__ live, const uint8_t* __restrict__ scol,
                                                               const uint8_t* __restrict__ rs_ok, uint8_t* __restrict__ schunks,
                                                               uint32_t* __restrict__ smasks, uint32_t* smargin, uint32_t* __restrict__ worked,
                                                               int c_margin, int e_max)
{
	if constexpr (LEGACY) return;                          // (as S3)
	constexpr uint32_t COL_MASK = ((1u << COL_CHUNKS) - 1u) << SYM_CHUNKS;
	const int g = blockIdx.x, k = g >> 1, d = g & 1;
	const uint32_t mask = live[g] ? smasks[g] : COL_MASK;
	if ((mask & COL_MASK) == COL_MASK) {                   // (uniform over the workgroup)
		if (threadIdx.x == 0) worked[g] = 0;
		return;
	}
	__shared__ float s_m[2][10];                           // ccm_used of captures k and k + 1
	if (threadIdx.x < 20) s_m[threadIdx.x / 10][threadIdx.x % 10] = ccm_used[(size_t)k * 10 + threadIdx.x];
	__syncthreads();
	uint32_t* mg = smargin + (size_t)g * NCELLS;
	for (int i = threadIdx.x; i < NCELLS; i += 256) {
		const int f = stitch_src(line_tab, axis, S, tears, strips, k, d, i);
		const float* m = s_m[f - k];
		uint32_t col[3];
		if (flood_flag[f] != 0) {
			const ushort2 xy = tb.cell_xy[i];
			const int x = (int)xy.x + drift[((size_t)f * NCELLS + i) * 2], y = (int)xy.y + drift[((size_t)f * NCELLS + i) * 2 + 1];
			mean6x6(rgb + (size_t)f * FRAME_RGB, x + 1, y + 1, col);
		} else {
			const uint32_t mv = cellmean[(size_t)f * GRID_CELLS + tb.cell_grid[i]];
			col[0] = mv & 0xFFu; col[1] = (mv >> 8) & 0xFFu; col[2] = (mv >> 16) & 0xFFu;
		}
		mg[i] = color_fit<true>((float)col[0], (float)col[1], (float)col[2], m, m[9] != 0.0f).margin;
	}
	if (threadIdx.x == 0) worked[g] = 1;
	__syncthreads();                                       // (the margins are read back below by other lanes of this workgroup)
	const uint8_t* cf = scol + (size_t)g * NCELLS;
	uint8_t* fc = schunks + (size_t)g * FRAME_BYTES;
	const uint32_t done = er_retry_blocks<int32_t, SYM_BLOCKS, COL_BLOCKS>(COL_MASK & ~mask, rs_ok + (size_t)g * ALL_BLOCKS, e_max, fc, [&](int b, int kb, bool ok) {
		const int sidx = (RS_BLOCK * (b - SYM_BLOCKS) + kb) * 4;
		int best = INT_MIN;
		uint32_t v = 0;
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const int cell = tb.stream_cell[sidx + q];
			v = (v << 2) | (cf[cell] & 3u);
			if (!ok) {
				const int sc = c_margin - (int)mg[cell];
				best = sc > best ? sc : best;
			}
		}
		return ErByte{v, best};
	});
	er_commit(mask | done, smasks + g, fc, SYM_CHUNKS, CHUNKS);
}
