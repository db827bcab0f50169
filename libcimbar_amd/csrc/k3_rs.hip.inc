// k3_rs.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K3: Reed-Solomon(155,125) decode
// ------------------------------------------------------------------------------------------------ K3 Reed-Solomon
// reed_solomon_stream.h:54-77 -> libcorrect decode.c:299-379, one 155-byte block per wavefront. The block is gathered
// straight out of the per-cell symbol (4 bit, 2 cells/byte) or colour (2 bit, 4 cells/byte) arrays through the inverse
// interleave map (Decoder.h:91-96,112; bitbuffer.h:62-84), so the 6200/3100-byte pre-RS streams never exist in memory.
// XOR of a 32-bit value over all 64 lanes (result uniform): 4 DPP butterflies inside each 16-lane row, then the four rows
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);    // quad_perm:[1,0,3,2]
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);    // quad_perm:[2,3,0,1]
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);   // row_half_mirror
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);   // row_mirror
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 16) ^
	       (uint32_t)__builtin_amdgcn_readlane((int)v, 32) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// ... over lanes 0..31 only (what the lanes above hold does not matter)
__device__ __forceinline__ uint32_t wave_xor32(uint32_t v)
{
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);
	v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
}

constexpr int RS_SYND = (RS_PARITY + 3) / 4 * 4;   // syndromes are stored four to a dword
constexpr int RS_POLY = 2 * RS_PARITY + 12;        // libcorrect's locator / previous-locator buffers (decode.c:259-297: min_distance + delay slack)
static_assert(RS_BLOCK <= 192, "a lane owns three bytes of the block");
struct RsShared {
	uint8_t exp[768];         // exp[512..767] = 0: where a zero byte's "logarithm" points, so that it contributes nothing
	uint8_t log[256];
	uint8_t enc[4][(RS_BLOCK + 7) / 8 * 8];      // block in transmit order
	__attribute__((aligned(4))) uint8_t synd[4][RS_SYND];
	uint8_t loc[4][RS_POLY];
	uint8_t last[4][RS_POLY];
};

// (templates over the LDS layout: k_rs_erasures' RsEraShared holds the same exp / log tables -- erasure.hip.inc)
template <class S> __device__ __forceinline__ uint8_t gf_mul(const S& s, uint8_t l, uint8_t r) { return (!l || !r) ? 0 : s.exp[(unsigned)s.log[l] + s.log[r]]; }
template <class S> __device__ __forceinline__ uint8_t gf_div(const S& s, uint8_t l, uint8_t r) { return (!l || !r) ? 0 : s.exp[255u + s.log[l] - s.log[r]]; }
// value of sum_i coef[i] * e^i for i <= order (polynomial.c:113-131 with element_exp rows = successive powers of e), e != 0
template <class S> __device__ __forceinline__ uint8_t gf_eval(const S& s, const uint8_t* coef, int order, uint8_t e)
{
	unsigned le = s.log[e] % 255u, acc = 0;   // log[1] == 255 -> 0
	uint8_t res = 0;
	for (int i = 0; i <= order; ++i) {
		if (coef[i]) res ^= s.exp[(unsigned)s.log[coef[i]] + acc];
		acc += le; if (acc >= 255u) acc -= 255u;
	}
	return res;
}

// the same with the coefficients' logarithms held one per lane in `lcoef` (512 for a zero coefficient: exp[512 + x] == 0): one table look-up
// per term instead of three dependent ones (coefficient, its logarithm, the product)
__device__ __forceinline__ uint8_t gf_eval_log(const RsShared& s, uint32_t lcoef, int order, uint8_t e)
{
	unsigned le = s.log[e] % 255u, acc = 0;   // log[1] == 255 -> 0
	uint32_t res = 0;
	for (int i = 0; i <= order; ++i) {
		res ^= s.exp[(uint32_t)__builtin_amdgcn_readlane((int)lcoef, i) + acc];
		acc += le; if (acc >= 255u) acc -= 255u;
	}
	return (uint8_t)res;
}

// NOSYND (timing probe only, CIMBAR_HIP_DEBUG_SKIP bit 128): the syndrome pass is left out and every block taken as a codeword -- right for clean
// frames, wrong otherwise; it bounds what ANY cheaper syndrome computation (bit-sliced, matrix cores, ...) could give the pipelined step.
// LIVE (the group decode, combine.hip.inc): *n_live frames of the nframes the grid covers are decoded, the workgroups past them return at once,
// and so do the wavefronts of a frame whose live_flag is 0.
template <int BITS, bool NOSYND = false, bool LIVE = false>   // 4: symbol stream, 2: colour stream, 6 | 7: the legacy modes' coupled stream (cells = symbols, cells2 = colours)
__global__ __launch_bounds__(256) void k_rs(const uint8_t* __restrict__ cells, Tables tb, int f0, int nframes, int first_chunk,
                                            uint8_t* __restrict__ chunks, uint8_t* __restrict__ rs_ok, int ok_offset, const uint8_t* __restrict__ cells2 = nullptr,
                                            const int* __restrict__ n_live = nullptr, const uint32_t* __restrict__ live_flag = nullptr)
{
	constexpr int NBLK0 = (BITS == 4) ? SYM_BLOCKS : (BITS == 2 ? COL_BLOCKS : ALL_BLOCKS), NBLK = NBLK0 > 0 ? NBLK0 : 1;
	constexpr int PER_BYTE = BITS >= 6 ? 1 : 8 / BITS;
	if constexpr (LIVE) {
		const int live = *n_live < nframes ? *n_live : nframes;
		if ((int)blockIdx.x * 4 >= live * NBLK) return;       // (uniform over the workgroup: before the barrier below)
		nframes = live;
	}
	__shared__ RsShared s;
	for (int k = threadIdx.x; k < 768; k += 256) s.exp[k] = k < 512 ? c_gf_exp[k] : (uint8_t)0;
	s.log[threadIdx.x] = c_gf_log[threadIdx.x];
	__syncthreads();

	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int gb = blockIdx.x * 4 + wv;                 // global block number over the batch
	const int b = gb % NBLK;
	if (gb / NBLK >= nframes) return;
	const int f = f0 + gb / NBLK;
	if constexpr (LIVE) { if (!live_flag[f]) return; }
	const uint8_t* cf = cells + (size_t)f * NCELLS;
	uint8_t* enc = s.enc[wv];

	// gather: stream byte B = 155*b + k packs stream cells PER_BYTE*B .. +PER_BYTE-1, first cell in the high bits.
	// Lane l owns bytes l, l+64, l+128 of the block (registers) and also parks them in LDS for the correction / output steps.
	uint32_t mine[3];
#pragma unroll
	for (int r = 0; r < 3; ++r) {
		const int k = lane + 64 * r;
		uint32_t v = 0;
		if (k < RS_BLOCK) {
			if constexpr (BITS >= 6) {
				// Decoder::do_decode_coupled (Decoder.h:121-161): stream cell s occupies bits [BITS*s, BITS*s + BITS) = colour | symbol(4);
				// stream byte B = bits [8B, 8B + 8) takes its bits from the two or three cells it overlaps
				const uint8_t* cf2 = cells2 + (size_t)f * NCELLS;
				const int bit0 = (RS_BLOCK * b + k) * 8, s0 = bit0 / BITS, off = bit0 - BITS * s0;
				uint32_t w = 0;
#pragma unroll
				for (int q = 0; q < 3; ++q) {
					const int sc = s0 + q < NCELLS ? s0 + q : NCELLS - 1;                 // (the third cell is only ever needed inside the stream)
					const int cell = tb.stream_cell[sc];
					w = (w << BITS) | ((uint32_t)(cf2[cell] & ((1u << (BITS - 4)) - 1u)) << 4) | (cf[cell] & 15u);
				}
				v = (w >> (3 * BITS - 8 - off)) & 0xFFu;
			} else {
				const int sidx = (RS_BLOCK * b + k) * PER_BYTE;
#pragma unroll
				for (int q = 0; q < PER_BYTE; ++q) v = (v << BITS) | (cf[tb.stream_cell[sidx + q]] & ((1u << BITS) - 1u));
			}
			enc[k] = (uint8_t)v;
		}
		mine[r] = v;
	}

	// syndromes S_j = r(alpha^(j+1)), r(x) = sum_i enc[154-i] x^i (decode.c:12-28), evaluated term-parallel: lane's byte k
	// contributes enc[k] * alpha^((j+1)*(154-k)); the 64 partial sums are XOR-reduced across the wave, four syndromes
	// (one per byte of a dword) at a time. No dependent chain of table look-ups, every lane busy.
	// Two roots at a time: P = (e_j, e_j+1) as packed u16, e_j = ((j+1) * (154-k)) mod 255; the next pair is P + 2*(154-k) mod 255,
	// reduced with one packed subtract + packed min (x >= 255 ? x - 255 : x  ==  min(x, x - 255) in unsigned 16-bit).
	typedef unsigned short us2 __attribute__((ext_vector_type(2)));
	uint32_t lgz[3];
	us2 P[3], step2[3];
#pragma unroll
	for (int r = 0; r < 3; ++r) {
		const int k = lane + 64 * r;
		const uint32_t sk = k < RS_BLOCK ? (uint32_t)(RS_BLOCK - 1 - k) : 0u;       // power of x this byte multiplies, < 255
		const uint32_t s2 = 2u * sk >= 255u ? 2u * sk - 255u : 2u * sk;
		lgz[r] = mine[r] ? (uint32_t)s.log[mine[r] & 0xFFu] : 512u;
		P[r] = us2{(unsigned short)sk, (unsigned short)s2};
		step2[r] = us2{(unsigned short)s2, (unsigned short)s2};
	}
	const us2 k255 = us2{255, 255};
	uint32_t any_nonzero = 0;
#pragma unroll
	for (int jg = 0; jg < (NOSYND ? 0 : (RS_PARITY + 3) / 4); ++jg) {
		uint32_t packed = 0;
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			if (4 * jg + 2 * h < RS_PARITY) {   // roots come in pairs; with an odd ecc_bytes the last pair's second root does not exist
				uint32_t part0 = 0, part1 = 0;
#pragma unroll
				for (int r = 0; r < 3; ++r) {
					part0 ^= s.exp[lgz[r] + P[r].x];
					part1 ^= s.exp[lgz[r] + P[r].y];
					P[r] += step2[r];
					P[r] = __builtin_elementwise_min(P[r], P[r] - k255);
				}
				if (4 * jg + 2 * h + 1 >= RS_PARITY) part1 = 0;
				packed |= (part0 | (part1 << 8)) << (16 * h);
			}
		}
		const uint32_t red = wave_xor(packed);
		any_nonzero |= red;
		if (lane == 0) reinterpret_cast<uint32_t*>(s.synd[wv])[jg] = red;
	}
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_s_waitcnt(0);   // LDS writes above visible to the wave's later reads
	const bool all_zero = any_nonzero == 0;

	int ok = 1;
	if (!all_zero) {
		uint8_t* loc = s.loc[wv];
		uint8_t* last = s.last[wv];
		const uint32_t vsynd = lane < RS_PARITY ? (uint32_t)s.synd[wv][lane] : 0u;
		// Berlekamp-Massey, decode.c:32-118. The control flow (discrepancy test, "room for more taps" test, orders, delay) is
		// libcorrect's, statement for statement; its array loops are element-wise, so lane k carries element k (and k+64) of
		// the locator / previous locator and all elements move at once. Entries above the loops' bounds keep their stale
		// values exactly as they do in libcorrect's buffers.
		for (int k = lane; k < RS_POLY; k += 64) { loc[k] = (k == 0); last[k] = (k == 0); }
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		unsigned loc_order = 0, last_order = 0, numerrors = 0, delay = 1;
		uint32_t llast_disc = 0;                        // log of the previous non-zero discrepancy used for an update (starts at 1: log 0, mod 255)
		// The discrepancy sum_{l=1..numerrors} loc[l] * S[i-l] is what every one of the 30 iterations computes, whether or not the locator
		// changes: it runs in the log domain out of registers -- lane j holds S[j] and log S[j] (512 for zero), lane l holds log loc[l]
		// (refreshed when the locator changes, a handful of times per block) -- so an iteration is ONE table look-up per lane. What lane l
		// multiplies with, log S[i - l], is last iteration's value of lane l - 1: one DPP wave shift, lane 0 taking log S[i] (no LDS permute).
		const uint32_t lsynd = vsynd ? (uint32_t)s.log[vsynd] : 512u;
		uint32_t lloc = lane == 0 ? 255u : 512u;        // log loc[lane] for lane < 64 (loc = 1: log[1] == 255 in libcorrect's table, exp[255 + x] == exp[x])
		uint32_t ls = 512u;
		// Once the locator is complete every remaining discrepancy is zero and the remaining iterations only count `delay` up -- for a block with e
		// errors that is 30 - 2e of the 30 iterations. Whether they ARE all zero is checked for all of them at once (lane i' computes the discrepancy
		// of iteration i' with the current locator: numerrors look-ups instead of a look-up and a wave reduce per iteration) after every update
		// of the second kind (no length change) that leaves 2 * numerrors <= i + 1 -- for e generic errors that is the update of iteration 2e - 1;
		// if so the loop ends there -- the locator, its order and numerrors are what libcorrect's loop would
		// leave behind (decode.c:32-118: a zero discrepancy changes nothing but `delay`, which nothing reads afterwards).
		auto rest_is_zero = [&](unsigned from) -> bool {
			uint32_t acc = vsynd, lsh = lsynd;
			for (unsigned l = 1; l <= numerrors; ++l) {
				lsh = from_left_lane(lsh, 512u);                                       // lane i': log S[i' - l]
				const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)lloc, (int)l);
				acc ^= s.exp[(li >= 512u || lsh >= 512u) ? 512u : li + lsh];
			}
			return __builtin_amdgcn_ballot_w64((unsigned)lane >= from && lane < RS_PARITY && (acc & 0xFFu) != 0u) == 0ull;
		};
		for (unsigned i = 0; i < (unsigned)RS_PARITY; ++i) {
			ls = from_left_lane(ls, (uint32_t)__builtin_amdgcn_readlane((int)lsynd, (int)i));      // lane l: log S[i - l] (lanes beyond i: masked below)
			uint32_t part_ = 0;
			if (lane >= 1 && (unsigned)lane <= numerrors) part_ = s.exp[ls >= 512u || lloc >= 512u ? 512u : lloc + ls];
			// (numerrors <= i + 1 <= RS_PARITY: with at most 31 taps everything that contributes sits in lanes 1 .. 31)
			const uint32_t red = RS_PARITY <= 31 ? wave_xor32(part_) : wave_xor(part_);
			const uint8_t disc = (uint8_t)(((uint32_t)__builtin_amdgcn_readlane((int)vsynd, (int)i) ^ red) & 0xFFu);
			if (!disc) { delay++; continue; }
			// last[.] * disc / last_disc for a non-zero element v of `last` is exp[log v + ld]: both factors' logarithms are wave-uniform
			// (the same field element as libcorrect's field_div(field_mul(v, disc), last_disc), decode.c:60-61,86-87)
			const uint32_t ld = ((uint32_t)__builtin_amdgcn_readfirstlane((int)s.log[disc]) + 255u - llast_disc) % 255u;
			auto scaled = [&](uint8_t v) -> uint8_t { return v ? s.exp[(uint32_t)s.log[v] + ld] : (uint8_t)0; };
			if (2 * numerrors <= i) {
				// last <- (last * disc / last_disc) shifted up by `delay`; then loc <- loc - last, last <- old loc, over [0, last_order + delay]
				uint8_t nloc[2] = {0, 0}, nlast[2] = {0, 0};
#pragma unroll
				for (int hh = 0; hh < 2; ++hh) {
					const unsigned k = (unsigned)lane + 64u * hh;
					if (k < (unsigned)RS_POLY) {
						const uint8_t oloc = loc[k], olast = last[k];
						const uint8_t shifted = k < delay ? (uint8_t)0
						                        : (k - delay <= last_order ? scaled(last[k - delay]) : olast);
						if (k <= last_order + delay) { nloc[hh] = oloc ^ shifted; nlast[hh] = oloc; }
						else { nloc[hh] = oloc; nlast[hh] = shifted; }
					}
				}
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_s_waitcnt(0);
#pragma unroll
				for (int hh = 0; hh < 2; ++hh) {
					const unsigned k = (unsigned)lane + 64u * hh;
					if (k < (unsigned)RS_POLY) { loc[k] = nloc[hh]; last[k] = nlast[hh]; }
				}
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
				__builtin_amdgcn_wave_barrier();
				lloc = nloc[0] ? (uint32_t)s.log[nloc[0]] : 512u;
				const unsigned t_order = loc_order;
				loc_order = last_order + delay;
				last_order = t_order;
				numerrors = i + 1 - numerrors;
				llast_disc = (ld + llast_disc) % 255u;      // log disc (mod 255)
				delay = 1;
				// (no end-of-work test here: 2 * old <= i gives 2 * numerrors >= i + 2, the locator cannot be complete right after a length change)
				continue;
			}
			// no more taps: loc[j + delay] -= last[j] * disc / last_disc for j <= last_order (last is not touched)
#pragma unroll
			for (int hh = 0; hh < 2; ++hh) {
				const unsigned k = (unsigned)lane + 64u * hh;
				if (k < (unsigned)RS_POLY && k >= delay && k - delay <= last_order) {
					const uint8_t v = loc[k] ^ scaled(last[k - delay]);
					loc[k] = v;
					if (hh == 0) lloc = v ? (uint32_t)s.log[v] : 512u;
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			loc_order = (last_order + delay > loc_order) ? last_order + delay : loc_order;
			delay++;
			if (2 * numerrors <= i + 1 && rest_is_zero(i + 1)) break;
		}
		const int order = (int)loc_order;
		__builtin_amdgcn_s_waitcnt(0);

		// error evaluator = locator * S mod x^30 (decode.c:149-161, polynomial.c:17-30): coefficient k on lane k
		// (order < RS_PARITY <= 64 wherever the results below are used, so lane i's lloc covers every coefficient that matters)
		uint32_t levalr = 512u;
		{
			uint32_t acc = 0, lsh = lsynd;                  // lsh: lane l holds log S[l - i] in iteration i (shifted one lane up per iteration)
			const int top = order < 63 ? order : 63;
			for (int i = 0; i <= top; ++i) {
				const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)lloc, i);
				if (i <= lane && lane < RS_PARITY && li < 512u && lsh < 512u) acc ^= s.exp[li + lsh];
				lsh = from_left_lane(lsh, 512u);
			}
			if (lane < RS_PARITY) levalr = acc ? (uint32_t)s.log[acc] : 512u;
		}
		// (its highest non-zero coefficient: the terms above contribute nothing to an evaluation -- exp[512 + x] == 0 -- so Forney's sum stops there)
		const unsigned long long evm = __builtin_amdgcn_ballot_w64(levalr < 512u);
		const int ev_top = evm ? 63 - (int)__builtin_clzll(evm) : -1;

		// Chien over every field element (decode.c:122-145); element 0 evaluates to loc[0] = 1, never a root. Lane l tests elements l, l+64, l+128,
		// l+192 side by side: four independent look-up chains per term instead of four loops in a row.
		// (order >= RS_PARITY would index past libcorrect's element_exp rows -- undefined there; treated as "no roots")
		unsigned long long rootm[4] = {0ull, 0ull, 0ull, 0ull};
		if (order < RS_PARITY) {
			uint32_t le4[4], acc4[4] = {0, 0, 0, 0}, res4[4] = {0, 0, 0, 0};
#pragma unroll
			for (int r = 0; r < 4; ++r) le4[r] = (uint32_t)s.log[(lane + 64 * r) & 0xFF] % 255u;       // (element 0: excluded below)
			for (int i = 0; i <= order; ++i) {
				const uint32_t lc = (uint32_t)__builtin_amdgcn_readlane((int)lloc, i);
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					res4[r] ^= s.exp[lc + acc4[r]];
					acc4[r] += le4[r]; acc4[r] = acc4[r] >= 255u ? acc4[r] - 255u : acc4[r];
				}
			}
#pragma unroll
			for (int r = 0; r < 4; ++r) rootm[r] = __builtin_amdgcn_ballot_w64((res4[r] & 0xFFu) == 0u && (lane + 64 * r) != 0);
		}
		const int n0 = (int)__popcll(rootm[0]), n1 = n0 + (int)__popcll(rootm[1]), n2 = n1 + (int)__popcll(rootm[2]), nroots = n2 + (int)__popcll(rootm[3]);
		if (nroots != order) {
			ok = 0;   // decode.c:354-358: too many errors
		} else {
			// the roots, compacted onto lanes 0 .. order-1 through the (now free) previous-locator buffer: one Forney pass for all of them
			{
				const unsigned long long below = (1ull << lane) - 1ull;
				const int base4[4] = {0, n0, n1, n2};
#pragma unroll
				for (int r = 0; r < 4; ++r)
					if ((rootm[r] >> lane) & 1ull) last[base4[r] + (int)__popcll(rootm[r] & below)] = (uint8_t)(lane + 64 * r);
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_s_waitcnt(0);
			// Forney (decode.c:165-196) + locations (decode.c:198-222) + fix-up (decode.c:366-369), one root per lane
			if (lane < nroots) {
				const uint8_t e = last[lane];
				// formal derivative (polynomial.c:74-87): der[i] = (i+1 odd) ? loc[i+1] : 0, order-1
				const uint8_t num = ev_top < 0 ? (uint8_t)0 : gf_eval_log(s, levalr, ev_top, e);       // = the sum over all RS_PARITY terms
				uint32_t den = 0;
				{
					unsigned le = s.log[e] % 255u, acc = 0;
					for (int i = 0; i <= order - 1; ++i) {
						if ((i + 1) & 1) den ^= s.exp[(uint32_t)__builtin_amdgcn_readlane((int)lloc, i + 1) + acc];
						acc += le; if (acc >= 255u) acc -= 255u;
					}
				}
				const uint8_t val = gf_div(s, num, (uint8_t)den);        // field_pow(root, fcr-1 = 0) == 1
				const uint8_t X = gf_div(s, 1, e);                        // error location = log(1/root); log(1) aliases to j = 0 -> 0
				const unsigned location = (X == 1) ? 0u : (unsigned)s.log[X];
				if (location < (unsigned)RS_BLOCK) enc[RS_BLOCK - 1 - location] ^= val;   // >= 155: lands in the zero padding, not emitted
			}
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_s_waitcnt(0);
		}
	}

	// the 125 message bytes of block b are bytes [125*(b%5), +125) of chunk first_chunk + b/5 (aligned_stream.h:62-85)
	uint8_t* dst = chunks + (size_t)f * FRAME_BYTES + (size_t)(first_chunk + b / BLOCKS_PER_CHUNK) * CHUNK + (size_t)(b % BLOCKS_PER_CHUNK) * RS_DATA;
	for (int k = lane; k < RS_DATA; k += 64) dst[k] = enc[k];
	if (lane == 0) rs_ok[(size_t)f * ALL_BLOCKS + ok_offset + b] = (uint8_t)ok;
}
