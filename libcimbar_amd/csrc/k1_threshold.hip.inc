// k1_threshold.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K1: threshold + bit-pack + colour means
// ------------------------------------------------------------------------------------------------ K1 threshold+pack
// CimbReader.cpp:30-46 preprocessSymbolGrid + bitmatrix.h:14-46, fused with the colour pass's pixel reads.
// One wavefront owns a full-width strip of pixel rows: lane l holds columns [PPL l, PPL l + PPL) and the wave walks down the
// strip, so every RGB byte is loaded from HBM exactly once (3 loads per lane per row, next rows prefetched while the
// current one is processed); the 5x5|7x7 box sums live in registers. PPL = K1_PPL pixels per lane: 16 (three 16-byte loads) for the
// 1024-pixel rows of modes 68 / 67 / 4 / 8, where 64 lanes x 16 is the row; 12 (three 12-byte loads) for mode 66's 736-pixel rows, which fill
// 46 lanes at 16 pixels each but 61 1/3 at 12 -- lane 61 holds the row's last four pixels, and the slots behind them are made copies of the last
// one (BORDER_REPLICATE of the box mean; for the sharpen filter's BORDER_REFLECT_101 the slot right behind it gets pixel W-2 first) by one
// v_perm_b32 per register with a per-lane selector, so that no lane but the last one does anything different.
//   gray  = (R*9798 + G*19235 + B*3735 + 2^14) >> 15                                 [assumed-OpenCV]
//   bit   = gray > round(box_sum / n)   <=>   n*gray > box_sum + n/2   (n = 25 | 49), BORDER_REPLICATE
// Output 1: plane[frame][row][32 words], pixel x -> word x/32, bit 31-(x%32).
// Output 2: cellmean[frame][112*112] = r | g<<8 | b<<16, the inner-6x6 mean (Cell.h:30-62: uint16 sums / 36) of every
//           cell at its UNDRIFTED grid position -- what read_color / init_ccm sample when no drift is in play
//           (CimbReader.cpp:133-137,216-217). Strips are aligned to the cell grid (56 strips x 2 cell rows), so a cell's
//           six inner rows always belong to one wave: per-byte column sums accumulate in registers over those rows and
//           are regrouped into cells through a 6 KiB LDS transpose once per cell row.
// Strip height is a trade: tall strips re-read few halo rows (2*RAD per strip) but 1024 frames x 16 strips = 5.33 "rounds" of
// the 3072 resident waves leave the chip partly idle while the last round drains; short strips drain evenly but re-read more.
// Measured on MI355X, 1024-frame batches: 16 strips 0.73 ms, 28: 0.73, 56: 0.68, 112: 0.80. A persistent-wave work queue mixing
// tall and short units was tried and lost to the plain grid (0.79 ms).
// TWO strip heights (round 5, profiles/r05h): the kernel's own time is the memory system's and is best with short strips (an even drain), but inside the
// pipelined loop -- where another batch's K1 and chain kernels fill the drain anyway -- what counts is how many vector instructions and halo rows K1
// spends per frame, because the chain kernels of the other batches in flight compete with it for issue slots (profiles/r05f): a strip of R cell rows
// runs ceil((9 R + 2 RAD) / RING) * RING row steps for 9 R rows of output, 24 for 18 at R = 2 (75 %) against 72 for 63 at R = 7 (87.5 %), and re-reads
// 2 RAD halo rows per strip. Same box, 1 024 frames per step: short strips K1 alone 0.667 ms / un-pipelined step 0.843 / pipelined step 0.779; seven
// cell rows 0.698 / 0.869 / **0.735** (four: 0.688 / 0.907 / 0.771; fourteen: 0.697 / 0.865 / 0.748; twenty-eight, one workgroup per frame: 0.702 / 0.873 / 0.779).
// So the pipelined entry point launches the TALL instance for batches that fill the chip with it, everything else the short one.
constexpr int k1_strips(int rows) { return (DIM_Y + rows - 1) / rows; }   // (the last strip may hold fewer cell rows: strips only have to begin on a cell row)
constexpr int k1_blocks(int rows) { return (k1_strips(rows) + 3) / 4; }    // four strips (wavefronts) per workgroup; a surplus wavefront of the last one returns at once
constexpr int K1_STRIPS = k1_strips(K1_CELLROWS);   // 2 (mode 66: 3) cell rows = 18 (27) pixel rows per strip (+ the margin at both ends of the frame): 56 | 39 | 23 strips
constexpr int K1_BLOCKS = k1_blocks(K1_CELLROWS), K1_TALL_BLOCKS = k1_blocks(K1_TALLROWS);
constexpr int GRID_CELLS = DIM_X * DIM_Y;

constexpr int K1_NP = K1_PPL / 2, K1_NDW = K1_PPL * 3 / 4;   // u16 pairs (pixel i | pixel i + NP << 16) and raw dwords per lane per row: 8, 12 | 6, 9
constexpr bool K1_PARTIAL = LAST_PX != K1_PPL;               // the last lane holds fewer than PPL pixels of the row
static_assert(K1_PPL == 16 || K1_PPL == 12, "16 pixels (3 x dwordx4) or 12 pixels (3 x dwordx3) per lane");
static_assert(!K1_PARTIAL || (K1_PPL == 12 && LAST_PX == 4), "a partial last lane holds exactly its first load (four pixels)");

// where a lane's three loads of a row start, as byte offsets into the row. Lanes beyond LAST_LANE idle: they load what LAST_LANE loads and their
// results are never read. A partial last lane (mode 66 at 12 pixels per lane: 4 of its 12 pixels exist) loads its first 12 bytes three times --
// never a byte beyond the row (the frame buffer ends with the last row) -- and patch_edge() below overwrites the slots that do not exist.
struct RowOff { uint32_t o0, o1, o2; };
__device__ __forceinline__ RowOff row_offsets(int lane)
{
	if (LAST_LANE != 63) lane = lane < LAST_LANE ? lane : LAST_LANE;
	RowOff r;
	r.o0 = (uint32_t)lane * (K1_PPL * 3);
	const bool whole = !K1_PARTIAL || lane < LAST_LANE;
	r.o1 = whole ? r.o0 + K1_PPL : r.o0;
	r.o2 = whole ? r.o0 + 2 * K1_PPL : r.o0;
	return r;
}
// Where a frame's rows come from. 16 pixels per lane: plain global loads from frame + row * pitch (the compiler keeps one 64-bit vector add per
// row and immediate offsets for the three loads). 12 pixels per lane: the three loads have three lane offsets, so the frame is a buffer resource
// and the row's byte offset the instruction's scalar offset -- buffer_load_dwordx3 v, voffset, s[rsrc], soffset: no vector address arithmetic at all
// (as global loads the compiler hoists the offsets' zero-extension out of the loop and then pays a 64-bit vector add per LOAD).
template <int PPL> struct RowSrc;
template <> struct RowSrc<16> {
	const uint8_t* frame;
	__device__ __forceinline__ explicit RowSrc(const uint8_t* f) : frame(f) {}
};
template <> struct RowSrc<12> {
	__amdgpu_buffer_rsrc_t rsrc;
	__device__ __forceinline__ explicit RowSrc(const uint8_t* f) : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(f), 0, (int)FRAME_RGB, 0x00020000)) {}
};
// (non-temporal loads, measured: with `nt` on these loads the kernel takes 1.15 ms instead of 0.68 -- a 128-byte line is a third each of three loads of
// one lane group, and only the default policy keeps it in the vector cache between them)
__device__ __forceinline__ void load_row(const RowSrc<16>& src, int r, const RowOff& ro, uint32_t (&d)[12])
{
	const uint4* p = reinterpret_cast<const uint4*>(src.frame + (size_t)r * (IMG_W * 3) + ro.o0);
	uint4 a = p[0], b = p[1], c = p[2];
	d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
	d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
	d[8] = c.x; d[9] = c.y; d[10] = c.z; d[11] = c.w;
}
__device__ __forceinline__ void load_row(const RowSrc<12>& src, int r, const RowOff& ro, uint32_t (&d)[9])
{
	typedef uint32_t u3 __attribute__((ext_vector_type(3)));
	const int so = __builtin_amdgcn_readfirstlane(r * (IMG_W * 3));   // (the row index is wave-uniform by construction)
	const u3 a = __builtin_amdgcn_raw_buffer_load_b96(src.rsrc, (int)ro.o0, so, 0);
	const u3 b = __builtin_amdgcn_raw_buffer_load_b96(src.rsrc, (int)ro.o1, so, 0);
	const u3 c = __builtin_amdgcn_raw_buffer_load_b96(src.rsrc, (int)ro.o2, so, 0);
	d[0] = a.x; d[1] = a.y; d[2] = a.z;
	d[3] = b.x; d[4] = b.y; d[5] = b.z;
	d[6] = c.x; d[7] = c.y; d[8] = c.z;
}

// PPL gray pixels straight from the raw dwords with v_dot4_u32_u8: pixel p starts at byte 3p; the dot product's fourth
// coefficient is 0, so the dword may carry the next pixel's first byte. The 15-bit coefficients are split c = hi*128 + lo
// (9798 = 76*128+70, 19235 = 150*128+35, 3735 = 29*128+23) and the low dot product is doubled, so that
//   T = (hi_dot << 8) + 2*lo_dot + 32768 = 2 * (R*9798 + G*19235 + B*3735 + 16384)   and   gray = T >> 16 = byte 2 of T.
// Leaving the result byte-aligned lets one v_perm_b32 pack two pixels into a u16 pair.
// BGR (captures stored B, G, R: extract.hip.inc): the R and B coefficients change places, nothing else.
template <int PPL, bool BGR = false>
__device__ __forceinline__ void gray_T(const uint32_t* d, uint32_t* T)
{
	constexpr uint32_t LO2 = BGR ? 46u | (70u << 8) | (140u << 16) : 140u | (70u << 8) | (46u << 16);
	constexpr uint32_t HI = BGR ? 29u | (150u << 8) | (76u << 16) : 76u | (150u << 8) | (29u << 16);
	constexpr int NDW = PPL * 3 / 4;
#pragma unroll
	for (int p = 0; p < PPL; ++p) {
		const int w = (3 * p) >> 2, sh = (3 * p) & 3;
		uint32_t v;
		// a pixel that starts at byte 1 of its dword still lies inside it: the coefficients move up a byte instead of the pixel moving down
		// (no v_alignbyte for pixels 3, 7, 11, 15 either: the kernel's own time is the memory system's, but every vector instruction it
		// does not issue is an issue slot for the chain kernels of the other batches in flight, profiles/r05f)
		const bool IN_PLACE = sh == 1;
		if (sh == 0 || IN_PLACE) v = d[w];
		else if (w == NDW - 1) v = d[NDW - 1] >> (8 * sh);
		else v = __builtin_amdgcn_alignbyte(d[w + 1], d[w], sh);
		const uint32_t lo = __builtin_amdgcn_udot4(v, IN_PLACE ? LO2 << 8 : LO2, 32768u, false);
		const uint32_t hi = __builtin_amdgcn_udot4(v, IN_PLACE ? HI << 8 : HI, 0u, false);
		T[p] = (hi << 8) + lo;
	}
}
// (the 16-pixel form by name: the capture kernels of extract.hip.inc hold 16 pixels per lane whatever the mode)
__device__ __forceinline__ void gray16_T(const uint32_t d[12], uint32_t T[16]) { gray_T<16>(d, T); }
// (pixel i | pixel i+NP << 16) from the byte-2 results of gray_T: one v_perm_b32 per pair
template <int NP>
__device__ __forceinline__ void pairs_T(const uint32_t* T, uint32_t* G)
{
#pragma unroll
	for (int i = 0; i < NP; ++i) G[i] = __builtin_amdgcn_perm(T[i + NP], T[i], 0x0c060c02u);   // bytes: [T_i.b2, 0, T_{i+NP}.b2, 0]
}
__device__ __forceinline__ void pairs_from_T(const uint32_t T[16], uint32_t G[8]) { pairs_T<8>(T, G); }

// lane l <- lane l-1 (lane 0 keeps `edge`), lane l <- lane l+1 (lane 63 keeps `edge`): DPP wave shifts, one VALU op each
__device__ __forceinline__ uint32_t from_left_lane(uint32_t v, uint32_t edge) { return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t from_right_lane(uint32_t v, uint32_t edge) { return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130, 0xf, 0xf, false); }
// the same where "the last lane" means the last lane of an image row (LAST_LANE): rows narrower than 1024 pixels end before lane 63
__device__ __forceinline__ uint32_t from_right_lane_row(uint32_t v, uint32_t edge)
{
	const uint32_t r = from_right_lane(v, edge);
	if (LAST_LANE == 63) return r;
	return (int)(threadIdx.x & 63) == LAST_LANE ? edge : r;
}


// The slots of a partial last lane that lie beyond the row (and all of the idle lanes behind it, which mirror it). sel_keep / sel_all are per-lane
// v_perm_b32 selectors, the identity on every other lane: see edge_selectors().
//   patch_reflect: BORDER_REFLECT_101 of the sharpen filter -- pixel W (slot LAST_PX) := pixel W-2, on the GRAY row, before it is filtered
//   patch_edge   : BORDER_REPLICATE of the box mean -- every slot from LAST_PX on := pixel W-1, on the row the box sums are taken of
struct EdgeSel { uint32_t keep_lo, all, reflect; };
__device__ __forceinline__ EdgeSel edge_selectors(int lane)
{
	EdgeSel e;
	const bool last = K1_PARTIAL && lane >= LAST_LANE;
	e.keep_lo = last ? 0x05040100u : 0x03020100u;   // [own lo half, the source's lo half]
	e.all = last ? 0x05040504u : 0x03020100u;       // [the source's lo half, twice]
	e.reflect = last ? 0x03020504u : 0x03020100u;   // [the source's lo half, own hi half]
	return e;
}
template <bool P = K1_PARTIAL, int LP = LAST_PX>
__device__ __forceinline__ void patch_reflect(uint32_t (&G)[K1_NP], const EdgeSel& e)
{
	if constexpr (P) {
		static_assert(LP >= 2 && LP < K1_NP, "pixels W-2 and W are low halves");
		G[LP] = __builtin_amdgcn_perm(G[LP - 2], G[LP], e.reflect);
	}
}
template <bool P = K1_PARTIAL, int LP = LAST_PX>
__device__ __forceinline__ void patch_edge(uint32_t (&G)[K1_NP], const EdgeSel& e)
{
	if constexpr (P) {
		const uint32_t src = G[LP - 1];           // pixel W-1 is its low half
#pragma unroll
		for (int i = 0; i < K1_NP; ++i) G[i] = __builtin_amdgcn_perm(src, G[i], i < LP ? e.keep_lo : e.all);
	}
}

// CimbReader.cpp:17-27 sharpen: filter2D with [0 -1 0; -1 4.5 -1; 0 -1 0], BORDER_REFLECT_101, saturate(round-half-even).
// On u16 pairs (pixel i | pixel i+NP << 16), the streaming path's layout: gn / gc / gs are the gray rows above, at and
// below the output row. Biased by 4096 per half so every intermediate stays a positive 16-bit field:
//   t' = 9c - 2(n+s+w+e) + 4096 in [2056, 6391];  q' = t' >> 1 (+1 if t' odd and q' odd: half -> even; 2048 keeps the parity);
//   result = clamp(q' - 2048, 0, 255).
__device__ __forceinline__ void sharp_pairs(const uint32_t (&gn)[K1_NP], const uint32_t (&gc)[K1_NP], const uint32_t (&gs)[K1_NP], uint32_t (&G)[K1_NP])
{
	typedef unsigned short us2 __attribute__((ext_vector_type(2)));
	constexpr int NP = K1_NP;
	// BORDER_REFLECT_101 at the row ends: pixel -1 -> pixel 1 (lane 0), pixel PPL of a full last lane -> pixel PPL-2 (a partial one: patch_reflect)
	const uint32_t W0 = from_left_lane(gc[NP - 1] >> 16, gc[1] & 0xFFFFu) | (gc[NP - 1] << 16);            // (pixel -1, pixel NP-1)
	const uint32_t E7 = (gc[0] >> 16) | (from_right_lane_row(gc[0] & 0xFFFFu, gc[NP - 2] >> 16) << 16);   // (pixel NP, pixel PPL)
#pragma unroll
	for (int i = 0; i < NP; ++i) {
		const uint32_t w = i == 0 ? W0 : gc[i - 1], e = i == NP - 1 ? E7 : gc[i + 1];
		const uint32_t sum = gn[i] + gs[i] + w + e;
		const uint32_t t = gc[i] * 9u + 0x10001000u - 2u * sum;
		uint32_t q = (t >> 1) & 0x7FFF7FFFu;
		q += t & q & 0x00010001u;
		us2 v = __builtin_bit_cast(us2, q);
		const us2 lo = {2048, 2048}, hi = {2048 + 255, 2048 + 255};
		v = __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi);
		G[i] = __builtin_bit_cast(uint32_t, v) - 0x08000800u;
	}
}

// One row of the streaming box-threshold. All per-pixel quantities travel as u16 pairs (pixel i | pixel i+NP << 16), i < NP,
// so a horizontal neighbour is simply the next register and plain 32-bit adds never carry between the halves.
//   ring : the last RING gray rows (RING = 2*RAD+2, even, so that the A/B prefetch buffers keep static roles)
//   C    : per-column sums of the newest 2*RAD+1 rows
// emit: row (y - RAD) has its full window -> PPL result bits for this lane, bit PPL-1-p = pixel p.
template <int RAD, int SLOT>
__device__ __forceinline__ uint32_t box_row(uint32_t (&ring)[2 * RAD + 2][K1_NP], uint32_t (&C)[K1_NP], const uint32_t (&G)[K1_NP], bool emit)
{
	constexpr int RING = 2 * RAD + 2, R = 2 * RAD + 1, N = R * R, NP = K1_NP;
	constexpr int OLD = (SLOT + 1) % RING;            // row y - (2*RAD+1), leaving the window
	constexpr int CTR = (SLOT + RING - RAD) % RING;   // row y - RAD, the one being emitted
#pragma unroll
	for (int i = 0; i < NP; ++i) {
		C[i] += G[i] - ring[OLD][i];
		ring[SLOT][i] = G[i];
	}
	if (!emit) return 0;

	// X[k] = pair register k - RAD, k = 0 .. NP + 2*RAD - 1: (pixel i, pixel i+NP) for i = -RAD .. NP-1+RAD
	uint32_t X[NP + 2 * RAD];
#pragma unroll
	for (int i = 0; i < NP; ++i) X[RAD + i] = C[i];
#pragma unroll
	for (int k = 1; k <= RAD; ++k) {
		// pixel -k comes from the left lane's pixel PPL-k (hi half of its C[NP-k]); BORDER_REPLICATE -> own pixel 0 on lane 0
		const uint32_t left = from_left_lane(C[NP - k] >> 16, C[0] & 0xFFFFu);
		X[RAD - k] = left | (C[NP - k] << 16);                       // (pixel -k, pixel NP-k)
		// pixel PPL-1+k comes from the right lane's pixel k-1 (lo half of its C[k-1]); replicate -> own pixel PPL-1 on a full last lane
		const uint32_t right = from_right_lane_row(C[k - 1] & 0xFFFFu, C[NP - 1] >> 16);
		X[RAD + NP - 1 + k] = (C[k - 1] >> 16) | (right << 16);      // (pixel NP-1+k, pixel PPL-1+k)
	}
	// KS = K - S, the constant of the comparison minus the sliding window sum: kept as ONE running value so that the comparison is a single
	// multiply-add (N * g + KS) instead of a multiply-add and a subtract
	constexpr uint32_t K = (0x8000u - (uint32_t)(N / 2) - 1u) * 0x00010001u;
	uint32_t KS = K;
#pragma unroll
	for (int k = 0; k < R; ++k) KS -= X[k];
	uint32_t M = 0;
#pragma unroll
	for (int i = 0; i < NP; ++i) {
		if (i > 0) KS += X[i - 1] - X[i + 2 * RAD];
		// N*g > S + N/2  <=>  bit 15 of (N*g + 0x8000 - N/2 - 1 - S), per half; no field under/overflows (|.| <= 12495)
		const uint32_t r = __umul24(ring[CTR][i], (uint32_t)N) + KS;
		M |= (r >> i) & (0x80008000u >> i);   // v_lshrrev + v_and_or
	}
	// pixel i < NP sits at bit 15-i, pixel i+NP at bit 31-i
	if constexpr (NP == 8) return (M & 0xFF00u) | (M >> 24);   // bit 15-p = pixel p
	else return ((M >> (16 - 2 * NP)) & (((1u << NP) - 1u) << NP)) | (M >> (32 - NP));   // bit 2NP-1-p = pixel p
}

// Between the prologue's row loads: keeps the compiler from interleaving the loads of different rows (it emits no instruction). The waits of the first
// pass count loads in issue order, and where the prologue's order differs from the loop's the compiler has to wait for the stricter of the two in
// every pass.
__device__ __forceinline__ void row_order_fence() { asm volatile("" ::: "memory"); }

template <int RAD, bool PRE, int ROWS = K1_CELLROWS>
#ifndef K1_WAVES
#define K1_WAVES 3
#endif
#ifndef K1_PRE_WAVES
#define K1_PRE_WAVES 2
#endif
#ifndef K1_PRE_DEPTH
#define K1_PRE_DEPTH 4
#endif
__global__ __launch_bounds__(256, PRE ? K1_PRE_WAVES : K1_WAVES) void k_threshold(const uint8_t* __restrict__ rgb, uint32_t* __restrict__ plane,
                                                                uint32_t* __restrict__ cellmean, uint32_t* __restrict__ flood_flag, int f0,
                                                                const int* __restrict__ sel, int sel_stride)
{
	constexpr int RING = 2 * RAD + 2;
	// per-frame choice of the variant (the extractor's verdict per capture, Extractor::NEEDS_SHARPEN == 2 -> the sharpening variant,
	// cimbar.cpp:147-154): both variants are launched over the batch and each keeps its own frames
	if (sel != nullptr && (sel[(size_t)(f0 + blockIdx.y) * sel_stride] == 2) != PRE) return;
	__shared__ __attribute__((aligned(16))) uint16_t s_col[4][64 * K1_PPL * 3];   // per-wave column sums of one cell row, by row byte (all 64 lanes write)
	constexpr int NP = K1_NP, NDW = K1_NDW;
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: keeps every row index / address base scalar
	const int strip = blockIdx.x * 4 + wave;
	constexpr int STRIPS = k1_strips(ROWS);
	if (strip >= STRIPS) return;   // (wave-uniform; the kernel has no workgroup barriers)
	const int f = f0 + blockIdx.y;
	const uint8_t* frame = rgb + (size_t)f * FRAME_RGB;
	uint32_t* out = plane + (size_t)f * PLANE_WORDS;
	uint32_t* cm = cellmean + (size_t)f * GRID_CELLS;
	const int y_begin = strip == 0 ? 0 : OFFSET + strip * ROWS * PITCH;
	const int y_end = strip == STRIPS - 1 ? IMG_H : OFFSET + (strip + 1) * ROWS * PITCH;
	const int total = (y_end - y_begin) + 2 * RAD;
	if (strip == 0 && lane == 0) flood_flag[f] = 0;   // per-frame state k_symbols accumulates into

	const RowOff ro = row_offsets(lane);
	const RowSrc<K1_PPL> src(frame);
	const EdgeSel es = edge_selectors(lane);
	uint32_t ring[RING][NP];
	uint32_t C[NP];
	uint32_t acc_e[NDW], acc_o[NDW];    // per-byte column sums over a cell's inner rows: even / odd bytes of each dword, u16 x2
#pragma unroll
	for (int k = 0; k < RING; ++k)
#pragma unroll
		for (int i = 0; i < NP; ++i) ring[k][i] = 0;
#pragma unroll
	for (int i = 0; i < NP; ++i) C[i] = 0;
#pragma unroll
	for (int k = 0; k < NDW; ++k) { acc_e[k] = 0; acc_o[k] = 0; }

	auto clampy = [](int y) { return y < 0 ? 0 : (y >= IMG_H ? IMG_H - 1 : y); };   // BORDER_REPLICATE of the thresholded source
	// Even strips walk down, odd strips walk up. A strip needs RAD rows of each neighbour; with alternating directions both
	// owners of a boundary touch it at the same moment (both at their start, or both at their end), so the halo rows are served
	// by L2 instead of being fetched from HBM a second time (measured: 21 % extra read traffic without this).
	const int dir = (strip & 1) ? -1 : 1;
	const int y_first = dir > 0 ? y_begin - RAD : y_end - 1 + RAD;     // first row visited
	const int y_stop = dir > 0 ? y_end - 1 + RAD : y_begin - RAD;      // last row visited
#ifndef K1_DEPTH
#define K1_DEPTH 3
#endif
	constexpr int DEPTH = PRE ? K1_PRE_DEPTH : K1_DEPTH;   // rows in flight per wave; RING % DEPTH == 0 keeps the buffer roles static after unrolling
	static_assert(RING % DEPTH == 0, "prefetch depth must divide the ring size");
	uint32_t buf[DEPTH][NDW];          // row t lives in buf[t % DEPTH] and is refilled with row t+DEPTH as soon as it is consumed
	auto bounded = [&](int y) { return clampy(dir > 0 ? (y < y_stop ? y : y_stop) : (y > y_stop ? y : y_stop)); };
	// PRE (sharpen): the row streamed at step t is the one AHEAD of the output row, reflect(yb(t) + dir) with yb = bounded(y):
	// sharpened row yb needs gray rows yb-1, yb, yb+1, kept in a 4-slot ring GR (slot = step mod 4; 4 divides RING, so roles stay static)
	auto ahead = [&](int t) {
		const int a = bounded(y_first + dir * t) + dir;
		return a < 0 ? 1 : (a >= IMG_H ? IMG_H - 2 : a);   // BORDER_REFLECT_101 of the sharpen filter
	};
	uint32_t GR[4][NP];
	if (PRE) {
		static_assert(!PRE || RING % 4 == 0, "gray ring period must divide the box ring");
		// slots 3 and 0 = the rows behind and at the first output row
		const int y0 = clampy(y_first), yb = y0 - dir;
		uint32_t d0[NDW], d1[NDW], T[K1_PPL];
		load_row(src, yb < 0 ? 1 : (yb >= IMG_H ? IMG_H - 2 : yb), ro, d0);
		load_row(src, y0, ro, d1);
#pragma unroll
		for (int k = 0; k < DEPTH; ++k) { load_row(src, ahead(k), ro, buf[k]); row_order_fence(); }
		gray_T<K1_PPL>(d0, T); pairs_T<NP>(T, GR[3]); patch_reflect(GR[3], es);
		gray_T<K1_PPL>(d1, T); pairs_T<NP>(T, GR[0]); patch_reflect(GR[0], es);
#pragma unroll
		for (int i = 0; i < NP; ++i) { GR[1][i] = 0; GR[2][i] = 0; }
	} else {
#pragma unroll
		for (int k = 0; k < DEPTH; ++k) { load_row(src, clampy(y_first + dir * k), ro, buf[k]); row_order_fence(); }
	}

	// One row step. `s` (the step's place in a pass over the ring) is a constant wherever this is called, so the ring slot, the prefetch buffer and the
	// gray-ring slots are fixed registers; the refill of the consumed buffer is an unconditional load.
	auto step = [&](const int s, const int t) __attribute__((always_inline)) {
		const int y = y_first + dir * t;
		uint32_t (&d)[NDW] = buf[s % DEPTH];
		uint32_t G[NP];
		int yl = y;   // the image row held in d
		if (PRE) {
			yl = ahead(t);
			uint32_t T[K1_PPL];
			gray_T<K1_PPL>(d, T);
			pairs_T<NP>(T, GR[(s + 1) & 3]);
			patch_reflect(GR[(s + 1) & 3], es);
			sharp_pairs(GR[(s + 3) & 3], GR[s & 3], GR[(s + 1) & 3], G);
			if (bounded(y + dir) == bounded(y)) {
				// the output row repeats (replicated border of the threshold source, or past the strip): re-seat the two
				// rows behind so the next step sees the same neighbourhood. Only the image's first / last strip gets here.
#pragma unroll
				for (int i = 0; i < NP; ++i) { GR[(s + 1) & 3][i] = GR[s & 3][i]; GR[s & 3][i] = GR[(s + 3) & 3][i]; }
			}
		} else {
			uint32_t T[K1_PPL];
			gray_T<K1_PPL>(d, T);
			pairs_T<NP>(T, G);
		}
		patch_edge(G, es);   // (a partial last lane: BORDER_REPLICATE of the row the box sums are taken of)

		// colour column sums: rows 9r+9 .. 9r+14 are the inner rows of cell row r (cell top = 8 + 9r)
		const bool in_grid = yl >= y_begin && yl < y_end && yl >= OFFSET + 1 && yl < OFFSET + DIM_Y * PITCH;
		const int ph = in_grid ? (yl - OFFSET) % PITCH : 0;
#ifdef K1_PROBE_NOCOLOR      // (timing probe only: the colour column sums and their transpose compiled out -- what K1 would take with ~20 % less vector work)
		if (false) {
#else
		if (ph >= 1 && ph <= 6) {
#endif
#pragma unroll
			for (int k = 0; k < NDW; ++k) {
				acc_e[k] += d[k] & 0x00FF00FFu;
				acc_o[k] += __builtin_amdgcn_perm(0u, d[k], 0x0c030c01u);   // (d >> 8) & 0x00FF00FF in one op
			}
		}
		// d is dead: refill it with the row DEPTH steps ahead
		load_row(src, PRE ? ahead(t + DEPTH) : bounded(y + dir * DEPTH), ro, d);

#ifdef K1_PROBE_NOCOLOR
		if (false) {
#else
		if (ph == (dir > 0 ? 6 : 1)) {   // the cell row's last inner row in walking order
#endif
			uint16_t* sc = s_col[wave];
			uint32_t w[2 * NDW];
#pragma unroll
			for (int k = 0; k < NDW; ++k) {
				w[2 * k] = (acc_e[k] & 0xFFFFu) | (acc_o[k] << 16);            // bytes 0,1 of dword k
				w[2 * k + 1] = (acc_e[k] >> 16) | (acc_o[k] & 0xFFFF0000u);    // bytes 2,3
				acc_e[k] = 0; acc_o[k] = 0;
			}
			if constexpr (K1_PPL == 16) {
				// 16-byte stores: a lane's row is 96 bytes, so lanes l and l+4 share their banks whatever the width; eight 4-byte pairs per lane
				// (what the compiler makes of 8-byte stores) cost four times the LDS cycles of six 16-byte ones (SQ_LDS_BANK_CONFLICT, profiles/r05m)
				// (by hand: the optimiser takes a vector store of four computed words apart again and pairs the pieces as ds_write2_b32. LDS operations of
				// one wavefront are issued and performed in order, so the reads below see these stores without the compiler knowing of them)
				typedef uint32_t u4 __attribute__((ext_vector_type(4)));
				const uint32_t at = (uint32_t)(uintptr_t)(sc + 48 * lane);   // (a shared-memory address' low word is its LDS offset)
#pragma unroll
				for (int j = 0; j < NDW / 2; ++j) {
					const u4 v = {w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
					asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(at), "v"(v), "n"(16 * j) : "memory");
				}
			} else {
				// (12 pixels per lane: rows of 72 bytes -- 8-byte stores, whose 16 lanes per pass fall on 16 different bank pairs; as 4-byte pieces four lanes share a bank)
				typedef uint32_t u2 __attribute__((ext_vector_type(2)));
				const uint32_t at = (uint32_t)(uintptr_t)(sc + K1_PPL * 3 * lane);
#pragma unroll
				for (int k = 0; k < NDW; ++k) {
					const u2 v = {w[2 * k], w[2 * k + 1]};
					asm volatile("ds_write_b64 %0, %1 offset:%2" :: "v"(at), "v"(v), "n"(8 * k) : "memory");
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			const int cell_row = (yl - OFFSET) / PITCH;
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				const int c = lane + 64 * half;
				if (c < DIM_X) {
					const uint16_t* src = sc + 3 * (PITCH * c + OFFSET + 1);   // first inner column of cell column c, as a row byte
					uint32_t r = 0, gg = 0, b = 0;
#pragma unroll
					for (int k = 0; k < 6; ++k) { r += src[3 * k]; gg += src[3 * k + 1]; b += src[3 * k + 2]; }
					cm[cell_row * DIM_X + c] = (r / 36u) | ((gg / 36u) << 8) | ((b / 36u) << 16);
				}
			}
			__builtin_amdgcn_wave_barrier();
		}

		uint32_t bits = 0;
		// (the first 2 RAD steps of a strip only fill the window: no row is complete yet, so the horizontal pass, the comparison and the bit gather
		// below are not issued for them -- a wave-uniform branch, 4 of a strip's 22 / 67 steps)
		const bool emit = t >= 2 * RAD;
		switch (s) {   // SLOT must be a compile-time constant; `s` is one after unrolling
			case 0: bits = box_row<RAD, 0>(ring, C, G, emit); break;
			case 1: bits = box_row<RAD, 1>(ring, C, G, emit); break;
			case 2: bits = box_row<RAD, 2>(ring, C, G, emit); break;
			case 3: bits = box_row<RAD, 3>(ring, C, G, emit); break;
			case 4: bits = box_row<RAD, 4>(ring, C, G, emit); break;
			case 5: bits = box_row<RAD, 5>(ring, C, G, emit); break;
			case 6: bits = box_row<RAD, 6 % RING>(ring, C, G, emit); break;
			default: bits = box_row<RAD, 7 % RING>(ring, C, G, emit); break;
		}
		if (emit) {
			uint32_t* orow = out + (size_t)(y - dir * RAD) * PLANE_ROW;   // the row whose window just completed
			if constexpr (K1_PPL == 16) {
				// gather the 8 x 16 bits of lanes 8k..8k+7 into lane 8k and store 16 bytes (columns 128k .. 128k+127 of the row)
				const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0xB1, 0xf, 0xf, true);   // lane^1
				const uint32_t w0 = (lane & 1) ? ((nb << 16) | bits) : ((bits << 16) | nb);                        // word of lanes (2j,2j+1), in both
				const uint32_t w1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w0, 0x4E, 0xf, 0xf, true);      // quad_perm:[2,3,0,1]: the quad's other word
				// lanes 4q..4q+3: lane 4q has w0 = word(2q), w1 = word(2q+1). Bring the next quad's two words over (row_shl:4).
				const uint32_t w2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w0, 0x104, 0xf, 0xf, true);     // row_shl:4 -> lane l gets lane l+4
				const uint32_t w3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w1, 0x104, 0xf, 0xf, true);
				if (!(lane & 7)) {
					uint4 v; v.x = w0; v.y = w1; v.z = w2; v.w = w3;
					*reinterpret_cast<uint4*>(orow + (lane >> 3) * 4) = v;
				}
			} else {
				// gather the 8 x 12 bits of lanes 8k..8k+7 into lane 8k and store 12 bytes (columns 96k .. 96k+95 of the row): pairs of lanes make
				// 24 bits, pairs of pairs 48 (as 16 + 32), and the two quads of the group the three words
				const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0xB1, 0xf, 0xf, true);    // lane^1
				const uint32_t c24 = (bits << 12) | nb;                                                             // lanes 2j: columns of lanes (2j, 2j+1)
				const uint32_t o24 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c24, 0x4E, 0xf, 0xf, true);    // quad_perm:[2,3,0,1]: the quad's other pair
				const uint32_t hi16 = c24 >> 8, lo32 = (c24 << 24) | o24;                                           // lanes 4q: the quad's 48 columns
				const uint32_t bh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi16, 0x104, 0xf, 0xf, true);   // row_shl:4 -> lane l gets lane l+4
				const uint32_t bl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo32, 0x104, 0xf, 0xf, true);
				if (!(lane & 7)) {
					struct __attribute__((packed, aligned(4))) W3 { uint32_t x, y, z; } v;
					v.x = (hi16 << 16) | (lo32 >> 16); v.y = (lo32 << 16) | bh; v.z = bl;
					*reinterpret_cast<W3*>(orow + (lane >> 3) * 3) = v;
				}
			}
		}
	};
	// FULL passes over the ring in a loop whose only exit is at its end, then the strip's last total % RING steps once more as straight-line code that
	// returns when the rows are done (2 of 24 steps of a short strip, 5 of 72 of a tall one used to run on clamped re-reads; the surplus steps issue
	// nothing now -- a scalar compare and a branch cost no vector issue slot, which is what the pipelined loop is short of, profiles/r05f).
	// Why not an exit test per step inside the loop: the body has lane-divergent branches (the two stores), so the compiler structurizes the whole loop
	// and routes every exit edge through a block it shares with the latch. The normal path then runs one such block per exit edge, each with a
	// vmcnt(0) -- the prefetch queue drained once per pass -- and copies of the buffer registers (DESIGN.md section 3, K1). With its one exit the loop is
	// straight-line: every step waits for the oldest row in flight only (vmcnt 3 DEPTH - 3 before its first use, 3 DEPTH before the last), step 0
	// included, because the prologue above issues its rows in walking order and so enters the loop with the queue the back edge carries.
	// (a strip holds at least one cell row, so there is always one full pass: the loop tests at its end, and no value has to survive around it)
	static_assert(PITCH + 2 * RAD >= RING, "a strip's shortest walk covers a full pass over the ring");
	int t0 = 0;
	do {
#pragma unroll
		for (int s = 0; s < RING; ++s) step(s, t0 + s);
		t0 += RING;
	} while (t0 + RING <= total);
#pragma unroll
	for (int s = 0; s < RING - 1; ++s) {
		if (t0 + s >= total) return;
		step(s, t0 + s);
	}
}
