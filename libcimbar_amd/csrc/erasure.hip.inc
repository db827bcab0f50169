// erasure.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace, after k3_rs.hip.inc and k4_frame.hip.inc).
// E3: Reed-Solomon errors-and-erasures decode of the mode's RS(RS_BLOCK, RS_DATA)
// ------------------------------------------------------------------------------------------------ E3 errors-and-erasures
// libcorrect's correct_reed_solomon_decode_with_erasures (decode.c:381-508) restated, one block per wavefront, for blocks whose erasure
// positions are given. Its quirks are kept: the location remap block_length - (pos + pad + 1) in 8-bit arithmetic (decode.c:424), the
// erasure locator prod (x + 1/X_i) (polynomial.c:161-197), the modified syndromes (erasure locator * S mod x^p, decode.c:247-257,445-452),
// Berlekamp-Massey over the remaining p - e of them (decode.c:32-118), Chien over the error locator alone with the erasure roots kept in
// front (decode.c:122-145), Forney over erasure locator * error locator with the ORIGINAL syndromes (decode.c:165-196, fcr = 1:
// field_pow(root, 0) == 1) and field_div(x, 0) == 0. e == 0 is libcorrect's errors-only decode, which the same arithmetic gives with an
// erasure locator of 1. e > p returns -1 (decode.c:392).
//
// The syndromes (of the received block and of the corrected one) and the Chien search run across the wavefront; the short serial parts
// (erasure locator, modified syndromes, Berlekamp-Massey, the polynomial products) run on lane 0, the Forney step one root per lane. The
// kernel is meant for the few blocks errors-only decoding could not correct, so it trades the last bit of speed for a line-by-line match.
//
// Where libcorrect's own behaviour is undefined -- a Berlekamp-Massey locator of order >= p, whose Chien search would read past the
// element_exp rows (decode.c:136), or erasure + error roots above p, whose Forney step would do the same (decode.c:194) -- the block is
// reported as a failure (-1).
//
// Per block: status -1 = libcorrect returns -1 (the message bytes written are the received ones, uncorrected); 0 = libcorrect returns the
// message length but the result fails the acceptance check; 1 = accepted. Acceptance: the corrected RS_BLOCK-byte word has all-zero
// syndromes, and no root of the combined locator lies in the shortened code's zero padding (location >= RS_BLOCK). libcorrect checks
// neither: it drops a correction in the padding and returns whatever the Forney step produced.
constexpr int ER_POLY = 2 * RS_PARITY + 12;   // locator / previous-locator scratch (as RS_POLY: libcorrect's min_distance + 1 and the shift slack)
struct RsEraShared {
	uint8_t exp[768];                          // exp[512..767] = 0, as in k_rs
	uint8_t log[256];
	uint8_t enc[4][192];                       // the block, transmit order; corrected in place
	uint8_t synd[4][64];                       // S_0 .. S_{p-1} of the received block
	uint8_t tsyn[4][64];                       // Berlekamp-Massey's input: modified syndromes e .. p-1
	uint8_t eloc[4][64];                       // erasure locator, order e
	uint8_t loc[4][ER_POLY];                   // Berlekamp-Massey's error locator
	uint8_t last[4][ER_POLY];                  // ... and its previous locator
	uint8_t full[4][2 * 64];                   // erasure locator * error locator
	uint8_t ev[4][64];                         // error evaluator = full * S mod x^p
	uint8_t roots[4][256];                     // erasure roots, then the Chien roots in increasing element order
	uint8_t val[4][64];                        // Forney values, one per root
	uint8_t where[4][64];                      // the roots' locations (power of x)
};
static_assert(RS_PARITY <= 64 && RS_BLOCK <= 192, "one lane per parity byte; a lane owns three bytes of the block");

// the block's p syndromes, S_j = r(alpha^(j+1)), r(x) = sum_k enc[RS_BLOCK-1-k] x^k, term-parallel over the lanes' three bytes; lane 0 writes
// them to `out` when it is not null. Returns whether all are zero (wave-uniform).
__device__ bool er_syndromes(RsEraShared& s, const uint8_t* enc, uint8_t* out, int lane)
{
	uint32_t lg[3], pw[3];
#pragma unroll
	for (int r = 0; r < 3; ++r) {
		const int k = lane + 64 * r;
		const uint32_t v = k < RS_BLOCK ? enc[k] : 0u;
		lg[r] = v ? (uint32_t)s.log[v] % 255u : 512u;
		pw[r] = k < RS_BLOCK ? (uint32_t)(RS_BLOCK - 1 - k) : 0u;
	}
	uint32_t any = 0;
	for (int j = 0; j < RS_PARITY; ++j) {
		uint32_t part = 0;
#pragma unroll
		for (int r = 0; r < 3; ++r) part ^= s.exp[lg[r] >= 512u ? 512u : lg[r] + (pw[r] * (uint32_t)(j + 1)) % 255u];
		const uint32_t sj = wave_xor(part) & 0xFFu;
		any |= sj;
		if (out && lane == 0) out[j] = (uint8_t)sj;
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	return any == 0;
}

// the decode of the block in s.enc[wv] with erasures at byte positions pos[0 .. e) (global or LDS); corrected in place. Returns the
// block's status (-1 / 0 / 1, see above); wave-uniform, all 64 lanes active. The enc bytes are visible to the whole wave on return.
__device__ int er_decode(RsEraShared& s, int wv, int lane, int e, const uint8_t* pos, int* nerr = nullptr)
{
	if (nerr) *nerr = 0;   // errors located beside the erasures (Berlekamp-Massey's locator order) where the decode gets that far
	uint8_t* enc = s.enc[wv];
	auto finish = [&](int st) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		return st;
	};
	if (e > RS_PARITY) return finish(-1);                  // decode.c:392

	uint8_t* synd = s.synd[wv];
	if (er_syndromes(s, enc, synd, lane)) return finish(1);  // decode.c:436-443: a codeword; nothing corrected

	uint8_t* eloc = s.eloc[wv];
	uint8_t* tsyn = s.tsyn[wv];
	uint8_t* loc = s.loc[wv];
	uint8_t* last = s.last[wv];
	uint8_t* full = s.full[wv];
	uint8_t* roots = s.roots[wv];
	int order = 0;
	bool bad = false;
	if (lane == 0) {
		// erasure roots (decode.c:422-428, 226-235): location L = block_length - (pos + pad + 1) as a field_logarithm_t, root = 1 / alpha^L
		const uint8_t* er = pos;
		for (int i = 0; i < e; ++i) {
			const uint8_t L = (uint8_t)(RS_BLOCK - 1 - (int)er[i]);
			roots[i] = gf_div(s, 1, s.exp[L]);
		}
		// erasure locator prod_i (x + root_i) (polynomial.c:161-197); e == 0: the constant 1 (the errors-only decode, decode.c:384-386)
		for (int k = 0; k <= RS_PARITY; ++k) eloc[k] = 0;
		if (e == 0) eloc[0] = 1;
		else {
			eloc[0] = roots[0]; eloc[1] = 1;
			for (int i = 1; i < e; ++i) {          // (x + root_i) * eloc, full product of order i + 1, from the top down in place
				for (int k = i + 1; k >= 0; --k) eloc[k] = (uint8_t)((k >= 1 ? eloc[k - 1] : 0) ^ gf_mul(s, roots[i], eloc[k]));
			}
		}
		// modified syndromes eloc * S mod x^p; Berlekamp-Massey reads entries e .. p-1 (decode.c:445-452)
		for (int k = 0; k < RS_PARITY; ++k) {
			uint32_t acc = 0;
			for (int i = 0; i <= e && i <= k; ++i) acc ^= gf_mul(s, eloc[i], synd[k - i]);
			if (k >= e) tsyn[k - e] = (uint8_t)acc;
		}
		// Berlekamp-Massey over p - e syndromes, statement for statement (decode.c:32-118)
		for (int k = 0; k < ER_POLY; ++k) { loc[k] = (k == 0); last[k] = (k == 0); }
		unsigned loc_order = 0, last_order = 0, numerrors = 0, delay = 1;
		uint32_t last_disc = 1;
		for (unsigned i = 0; i < (unsigned)(RS_PARITY - e); ++i) {
			uint32_t disc = tsyn[i];
			for (unsigned j = 1; j <= numerrors; ++j) disc ^= gf_mul(s, loc[j], tsyn[i - j]);
			if (!disc) { delay++; continue; }
			if (2 * numerrors <= i) {
				for (int j = (int)last_order; j >= 0; --j)
					if ((unsigned)j + delay < (unsigned)ER_POLY) last[j + delay] = gf_div(s, gf_mul(s, last[j], disc), last_disc);
				for (int j = (int)delay - 1; j >= 0; --j) if (j < ER_POLY) last[j] = 0;
				for (unsigned j = 0; j <= last_order + delay && j < (unsigned)ER_POLY; ++j) {
					const uint8_t t = loc[j];
					loc[j] ^= last[j];
					last[j] = t;
				}
				const unsigned t_order = loc_order;
				loc_order = last_order + delay;
				last_order = t_order;
				numerrors = i + 1 - numerrors;
				last_disc = disc;
				delay = 1;
				continue;
			}
			for (int j = (int)last_order; j >= 0; --j)
				if ((unsigned)j + delay < (unsigned)ER_POLY) loc[j + delay] ^= gf_div(s, gf_mul(s, last[j], disc), last_disc);
			loc_order = (last_order + delay > loc_order) ? last_order + delay : loc_order;
			delay++;
		}
		order = (int)loc_order;
		bad = order >= RS_PARITY || order + e > RS_PARITY;   // libcorrect's look-up rows end there (see above)
	}
	order = __builtin_amdgcn_readfirstlane(order);
	bad = __builtin_amdgcn_readfirstlane((int)bad) != 0;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	if (nerr) *nerr = order;
	if (bad) return finish(-1);

	// Chien over all 256 field elements with the error locator alone (decode.c:122-145); element 0 evaluates to loc[0] = 1, never a root.
	// Lane l tests elements l, l+64, l+128, l+192; the roots land in increasing element order behind the e erasure roots.
	unsigned long long rootm[4];
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const int x = lane + 64 * r;
		rootm[r] = __builtin_amdgcn_ballot_w64(x != 0 && gf_eval(s, loc, order, (uint8_t)x) == 0);
	}
	const int n0 = (int)__popcll(rootm[0]), n1 = n0 + (int)__popcll(rootm[1]), n2 = n1 + (int)__popcll(rootm[2]), nroots = n2 + (int)__popcll(rootm[3]);
	if (nroots != order) return finish(-1);           // decode.c:474-479: too many errors
	{
		const unsigned long long below = (1ull << lane) - 1ull;
		const int base4[4] = {0, n0, n1, n2};
#pragma unroll
		for (int r = 0; r < 4; ++r)
			if ((rootm[r] >> lane) & 1ull) roots[e + base4[r] + (int)__popcll(rootm[r] & below)] = (uint8_t)(lane + 64 * r);
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();

	// combined locator = erasure locator * error locator (decode.c:481-484) and the error evaluator = combined * S mod x^p (decode.c:175-179)
	const int total = e + order;
	uint8_t* ev = s.ev[wv];
	if (lane == 0) {
		for (int k = 0; k <= total; ++k) {
			uint32_t acc = 0;
			for (int i = 0; i <= e && i <= k; ++i) if (k - i <= order) acc ^= gf_mul(s, eloc[i], loc[k - i]);
			full[k] = (uint8_t)acc;
		}
		for (int k = 0; k < RS_PARITY; ++k) {
			uint32_t acc = 0;
			for (int i = 0; i <= total && i <= k; ++i) acc ^= gf_mul(s, full[i], synd[k - i]);
			ev[k] = (uint8_t)acc;
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();

	// Forney (decode.c:165-196) and the locations (decode.c:198-222), one root per lane. The formal derivative's coefficient i is
	// full[i + 1] for even i, 0 for odd i (polynomial.c:74-87).
	uint8_t* val = s.val[wv];
	uint8_t* where = s.where[wv];
	if (lane < total) {
		const uint8_t x = roots[lane];
		const uint8_t num = gf_eval(s, ev, RS_PARITY - 1, x);
		uint32_t den = 0;
		{
			const unsigned lx = s.log[x] % 255u;
			unsigned acc = 0;
			for (int i = 0; i <= total - 1; ++i) {
				if (!(i & 1) && full[i + 1]) den ^= s.exp[(unsigned)s.log[full[i + 1]] % 255u + acc];
				acc += lx; if (acc >= 255u) acc -= 255u;
			}
		}
		val[lane] = gf_div(s, num, den);
		const uint8_t X = gf_div(s, 1, x);                     // the location is log(1 / root); 1 is found at j = 0 first: location 0
		where[lane] = X == 1 ? (uint8_t)0 : s.log[X];
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// the corrections in libcorrect's order (two roots may share a location); a location >= RS_BLOCK is the zero padding: not emitted
	int in_pad = 0;
	if (lane == 0) {
		for (int i = 0; i < total; ++i) {
			const int w = where[i];
			if (w < RS_BLOCK) enc[RS_BLOCK - 1 - w] ^= val[i];
			else in_pad = 1;
		}
	}
	in_pad = __builtin_amdgcn_readfirstlane(in_pad);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	const bool clean = er_syndromes(s, enc, nullptr, lane);
	return finish(clean && !in_pad ? 1 : 0);
}

__device__ __forceinline__ void er_tables(RsEraShared& s)
{
	for (int k = threadIdx.x; k < 768; k += 256) s.exp[k] = k < 512 ? c_gf_exp[k] : (uint8_t)0;
	s.log[threadIdx.x] = c_gf_log[threadIdx.x];
	__syncthreads();
}

// cimbar_hip_rs_decode_erasures. blocks: [n][RS_BLOCK]; erasures: [n][RS_BLOCK], row b's first counts[b] bytes are byte positions in the
// block; msgs: [n][RS_DATA] (libcorrect's output, the received bytes where it fails)
__global__ __launch_bounds__(256) void k_rs_erasures(const uint8_t* __restrict__ blocks, int n, const uint8_t* __restrict__ erasures,
                                                     const uint8_t* __restrict__ counts, uint8_t* __restrict__ msgs, int8_t* __restrict__ status)
{
	__shared__ RsEraShared s;
	er_tables(s);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int b = blockIdx.x * 4 + wv;
	if (b >= n) return;
	uint8_t* enc = s.enc[wv];
	for (int k = lane; k < RS_BLOCK; k += 64) enc[k] = blocks[(size_t)b * RS_BLOCK + k];
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	const int st = er_decode(s, wv, lane, counts[b], erasures + (size_t)b * RS_BLOCK);
	for (int k = lane; k < RS_DATA; k += 64) msgs[(size_t)b * RS_DATA + k] = enc[k];
	if (lane == 0) status[b] = (int8_t)st;
}

// ------------------------------------------------------------------------------------------------ the erasure retry
constexpr int ERASURE_SLACK = 6;
// the selection every retry shares: the rank of each flagged byte (score > 0) among the flagged ones, higher score first, then lower position;
// the e_max best become erasures, pos[rank] = byte position. One wavefront per block; returns the erasure count (wave-uniform), pos visible
// to the wave.
template <class T>
__device__ __forceinline__ int er_select(const T* score, int lane, int e_max, uint8_t* pos)
{
	int mine = 0;
	for (int k = lane; k < RS_BLOCK; k += 64) {
		const int sk = score[k];
		if (sk <= 0) continue;
		int rank = 0;
		for (int q = 0; q < RS_BLOCK; ++q) {
			const int sq = score[q];
			rank += (sq > sk || (sq == sk && q < k)) ? 1 : 0;
		}
		if (rank < e_max) { pos[rank] = (uint8_t)k; ++mine; }
	}
	for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	return mine;
}

// The retry itself, for one frame or group and a workgroup of four wavefronts (all 256 threads call it): the wavefronts take the blocks
// [B_FIRST, B_FIRST + NB) -- whole chunks -- of the chunks in `todo`, a block each at a time. gather(b, k, ok) gives stream byte k of block b
// and, for a block errors-only decoding failed (!ok = rs_ok[b] == 0; the score of a decoded block is not read), its score: flagged when > 0.
// It is all that differs between the callers. T is the type of a score row in LDS.
//  * a failed block is decoded again with the e_max best-scored flagged bytes as erasures (er_select); none flagged: not retried, status -2
//    (it would be errors-only again)
//  * a block errors-only decoding accepted is decoded again with none: libcorrect's errors-only result (its chunk's slot has been zeroed)
//  * status: er_decode's -1 / 0 / 1, and 1 only within the slack rule below; an accepted block's RS_DATA bytes go to its place in its chunk's
//    slot under `fc`
// Returns, uniform over the workgroup, the chunks of `todo` whose blocks were all accepted. The status of a block outside `todo` is neither
// written nor read; nothing but the accepted blocks' bytes is written to global memory.
// The LDS is the routine's own and it returns without a barrier behind its last read: call it at most once per kernel, or barrier between calls.
struct ErByte { uint32_t byte; int score; };
template <class T, int B_FIRST, int NB, class Gather>
__device__ __forceinline__ uint32_t er_retry_blocks(uint32_t todo, const uint8_t* __restrict__ rs_ok, int e_max, uint8_t* __restrict__ fc, Gather gather)
{
	static_assert(B_FIRST % BLOCKS_PER_CHUNK == 0 && NB % BLOCKS_PER_CHUNK == 0, "whole chunks");
	__shared__ RsEraShared s;
	__shared__ T s_score[4][192];
	__shared__ uint8_t s_pos[4][64];
	__shared__ int8_t s_st[NB > 0 ? NB : 1];
	__shared__ uint32_t s_done;
	er_tables(s);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	for (int b = B_FIRST + wv; b < B_FIRST + NB; b += 4) {
		const int j = b / BLOCKS_PER_CHUNK;
		if (!(todo & (1u << j))) continue;
		const bool ok = rs_ok[b] != 0;
		uint8_t* enc = s.enc[wv];
		T* score = s_score[wv];
		for (int k = lane; k < RS_BLOCK; k += 64) {
			const ErByte g = gather(b, k, ok);
			enc[k] = (uint8_t)g.byte;
			score[k] = (T)g.score;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		int e = 0;
		if (!ok) {
			e = er_select(score, lane, e_max, s_pos[wv]);
			if (e == 0) { if (lane == 0) s_st[b - B_FIRST] = -2; continue; }   // nothing to erase: errors-only already failed it
		}
		int nerr = 0;
		int st = er_decode(s, wv, lane, e, s_pos[wv], &nerr);
		// a retried block must also leave ERASURE_SLACK syndromes unused: a damaged block lies within s errors of SOME codeword on its n - e
		// unerased bytes with probability ~ C(n - e, s) 255^s / 256^(p - e), which the codeword check cannot see (1 in 200 blocks at
		// p - e = 8, s = 4); with 2 s <= p - e - 6 it is below 1e-14
		if (st == 1 && e > 0 && 2 * nerr > RS_PARITY - e - ERASURE_SLACK) st = 0;
		if (st == 1) {
			uint8_t* dst = fc + (size_t)j * CHUNK + (size_t)(b % BLOCKS_PER_CHUNK) * RS_DATA;
			for (int k = lane; k < RS_DATA; k += 64) dst[k] = enc[k];
		}
		if (lane == 0) s_st[b - B_FIRST] = (int8_t)st;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t done = 0;
		for (int j = B_FIRST / BLOCKS_PER_CHUNK; j < (B_FIRST + NB) / BLOCKS_PER_CHUNK; ++j) {
			if (!(todo & (1u << j))) continue;
			bool all = true;
			for (int q = 0; q < BLOCKS_PER_CHUNK; ++q) all = all && s_st[j * BLOCKS_PER_CHUNK + q - B_FIRST] == 1;
			if (all) done |= 1u << j;
		}
		s_done = done;
	}
	__syncthreads();
	return s_done;
}

// what the frame retries and the group colour retry do with the result: the mask `m` (the old one and the chunks the retry added) is written,
// and the slots of the chunks [j0, j1) it still lacks are zeroed again
__device__ __forceinline__ void er_commit(uint32_t m, uint32_t* __restrict__ mask_out, uint8_t* __restrict__ fc, int j0, int j1)
{
	if (threadIdx.x == 0) *mask_out = m;
	for (int j = j0; j < j1; ++j)
		if (!(m & (1u << j)))
			for (int k = threadIdx.x; k < CHUNK; k += 256) fc[(size_t)j * CHUNK + k] = 0;
}

// ------------------------------------------------------------------------------------------------ symbol erasure retry of a decoded frame
// Opt-in (cimbar_hip_set_erasure_decode), launched after k_frame_end on the same stream, one workgroup per frame, modes 68 / 67 / 66.
// A frame whose symbol chunks are all in the mask returns at once (a clean batch costs one launch). Otherwise the four waves walk the symbol
// blocks of the chunks the mask lacks:
//  * confidence: d_sym(c) = popcount(ahash8 at the cell's final position ^ tile hash of its decoded symbol), from the bit plane, the drift and
//    the symbol the decode produced (the position is the cell's grid position plus its drift where the frame went through the flood pass --
//    the window k_colors reads -- and the grid position otherwise). Where the +-7 drift clamp moved the final position off the matched
//    window this definition wins.
//  * selection: a stream byte comes from two cells (nibbles); its score is max over them of d_sym - T_sym + 1, and it is flagged when the
//    score is > 0. The max_erasures highest scores are kept, ties to the lower byte position.
//  * a block errors-only decoding failed is retried with those erasures (none flagged: not retried -- it would be errors-only again); a
//    block it decoded is decoded again with none (libcorrect's errors-only result, because k_frame_end has zeroed the slots of the chunks the
//    mask lacks). Then a chunk whose blocks are now all accepted (status 1) gets its bytes and its mask bit; the slots of chunks still
//    missing are zeroed again (er_retry_blocks, er_commit). Chunks already in the mask, the colour chunks, rs_ok, the frame state and the
//    colour-correction carry are not touched. (The colour chunks have a retry of their own: k_colour_erasure_frame below.)
__global__ __launch_bounds__(256) void k_erasure_frame(const uint32_t* __restrict__ plane, Tables tb, const uint8_t* __restrict__ symbols,
                                                       const int8_t* __restrict__ drift, const uint32_t* __restrict__ flood_flag,
                                                       const uint8_t* __restrict__ rs_ok, uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks,
                                                       int f0, int t_sym, int e_max)
{
	if constexpr (LEGACY) return;                          // (one coupled stream: no symbol-only blocks; the host never launches it there)
	constexpr uint32_t SYM_MASK = (1u << SYM_CHUNKS) - 1u;
	const int f = f0 + blockIdx.x;
	const uint32_t mask = masks[f];
	if ((mask & SYM_MASK) == SYM_MASK) return;             // (uniform over the workgroup)
	const uint8_t* sym = symbols + (size_t)f * NCELLS;
	const uint32_t* pl = plane + (size_t)f * PLANE_WORDS;
	const bool flooded = flood_flag[f] != 0;
	uint8_t* fc = chunks + (size_t)f * FRAME_BYTES;
	const uint32_t done = er_retry_blocks<int16_t, 0, SYM_BLOCKS>(SYM_MASK & ~mask, rs_ok + (size_t)f * ALL_BLOCKS, e_max, fc, [&](int b, int k, bool ok) {
		const int sidx = (RS_BLOCK * b + k) * 2;
		int best = -32768;
		uint32_t v = 0;
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			const int cell = tb.stream_cell[sidx + q];
			const uint32_t sy = sym[cell] & 15u;
			v = (v << 4) | sy;
			if (!ok) {
				const ushort2 xy = tb.cell_xy[cell];
				const int dx = flooded ? drift[((size_t)f * NCELLS + cell) * 2] : 0, dy = flooded ? drift[((size_t)f * NCELLS + cell) * 2 + 1] : 0;
				uint32_t rows[10];
				window_rows(pl, (int)xy.x + dx - 1, (int)xy.y + dy - 1, rows);
				const int d = (int)__popcll(window_hash(rows, 4) ^ c_tile[sy]);
				best = d - t_sym + 1 > best ? d - t_sym + 1 : best;
			}
		}
		return ErByte{v, best};
	});
	er_commit(mask | done, masks + f, fc, 0, SYM_CHUNKS);
}

// ------------------------------------------------------------------------------------------------ colour erasure retry of a decoded frame
// Opt-in (cimbar_hip_set_colour_erasure_decode), launched after k_frame_end (and after k_erasure_frame where that runs) on the same stream, one
// workgroup of four wavefronts per frame, modes 68 / 67 / 66. A frame whose colour chunks are all in the mask returns at once (worked[f] = 0:
// CIMBAR_HIP_TAP_COLOUR_MARGIN reports 0xFFFFFFFF for its cells). Otherwise:
//  * confidence: margin(c) = (second-smallest) - (smallest) squared distance of get_best_color (color_fit<true>), from exactly what k_colors
//    classified the cell from -- the K1 cell mean where the frame did not go through the flood pass, mean6x6 at the drifted position where it
//    did, and the matrix in force (ccm_used[f], active flag included). The workgroup computes it for every cell of the frame once, into
//    margins[f] (the tap).
//  * selection: a colour-stream byte comes from four cells (2 bits each); its score is max over them of c_margin - margin(c), flagged when the
//    score is > 0. The e_max highest scores are kept, ties to the lower byte position.
//  * retry, acceptance and the mask update are er_retry_blocks and er_commit over the colour blocks: a colour chunk whose blocks are all
//    accepted gets its bytes and its mask bit; the slots of colour chunks still missing are zeroed again. Chunks already in the mask, the
//    symbol chunks, rs_ok, the frame state, the colours and the colour-correction carry are not touched.
__global__ __launch_bounds__(256) void k_colour_erasure_frame(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                              const uint8_t* __restrict__ colors, const int8_t* __restrict__ drift,
                                                              const uint32_t* __restrict__ flood_flag, const float* __restrict__ ccm_used,
                                                              const uint8_t* __restrict__ rs_ok, uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks,
                                                              uint32_t* margins, uint32_t* __restrict__ worked, int f0, int c_margin, int e_max)
{
	if constexpr (LEGACY) return;                          // (one coupled stream: no colour-only blocks; the host never launches it there)
	constexpr uint32_t COL_MASK = ((1u << COL_CHUNKS) - 1u) << SYM_CHUNKS;
	const int f = f0 + blockIdx.x;
	const uint32_t mask = masks[f];
	if ((mask & COL_MASK) == COL_MASK) {                   // (uniform over the workgroup)
		if (threadIdx.x == 0) worked[f] = 0;
		return;
	}
	__shared__ float s_m[10];
	if (threadIdx.x < 10) s_m[threadIdx.x] = ccm_used[(size_t)f * 10 + threadIdx.x];
	__syncthreads();
	const bool flooded = flood_flag[f] != 0;
	const bool active = s_m[9] != 0.0f;
	uint32_t* mg = margins + (size_t)f * NCELLS;
	for (int i = threadIdx.x; i < NCELLS; i += 256) {
		uint32_t col[3];
		if (flooded) {
			const ushort2 xy = tb.cell_xy[i];
			const int x = (int)xy.x + drift[((size_t)f * NCELLS + i) * 2], y = (int)xy.y + drift[((size_t)f * NCELLS + i) * 2 + 1];
			mean6x6(rgb + (size_t)f * FRAME_RGB, x + 1, y + 1, col);
		} else {
			const uint32_t mv = cellmean[(size_t)f * GRID_CELLS + tb.cell_grid[i]];
			col[0] = mv & 0xFFu; col[1] = (mv >> 8) & 0xFFu; col[2] = (mv >> 16) & 0xFFu;
		}
		mg[i] = color_fit<true>((float)col[0], (float)col[1], (float)col[2], s_m, active).margin;
	}
	if (threadIdx.x == 0) worked[f] = 1;
	__syncthreads();                                       // (the margins are read back below by other lanes of this workgroup)
	const uint8_t* cf = colors + (size_t)f * NCELLS;
	uint8_t* fc = chunks + (size_t)f * FRAME_BYTES;
	const uint32_t done = er_retry_blocks<int32_t, SYM_BLOCKS, COL_BLOCKS>(COL_MASK & ~mask, rs_ok + (size_t)f * ALL_BLOCKS, e_max, fc, [&](int b, int k, bool ok) {
		const int sidx = (RS_BLOCK * (b - SYM_BLOCKS) + k) * 4;
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
	er_commit(mask | done, masks + f, fc, SYM_CHUNKS, CHUNKS);
}
