// k4_frame.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// K4/K5/K7: chunk bookkeeping, colour-correction matrix, colour classifier
// ------------------------------------------------------------------------------------------------ per-frame glue
// FountainMetadata.h:16-92
__device__ __forceinline__ uint32_t md_id(const uint8_t h[6]) { return (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24); }
__device__ __forceinline__ unsigned md_file_size(const uint8_t h[6]) { return (unsigned)h[3] | ((unsigned)h[2] << 8) | ((unsigned)h[1] << 16) | (((unsigned)h[0] & 0x80u) << 17); }
__device__ __forceinline__ void md_increment(uint8_t h[6], unsigned radioactive)
{
	unsigned next = ((unsigned)h[5] | ((unsigned)h[4] << 8)) + 1;
	if (next == radioactive) next += 1;
	h[4] = (uint8_t)((next >> 8) & 0xFF);
	h[5] = (uint8_t)(next & 0xFF);
}

struct FrameState {           // aligned_stream state carried from the symbol to the colour pass
	uint32_t offset;          // aligned_stream::_offset
	uint32_t bad;             // aligned_stream::_badChunk
	uint32_t mask;            // chunks delivered so far (aligned_stream::_totalCount == 625 * popcount(mask))
	uint32_t pad;
};

// aligned_stream.h:39-119 driven one 125-byte RS block at a time (reed_solomon_stream.h:62-74,109-114). A bad LAST block of
// a chunk leaves _badChunk set, so the NEXT chunk is the one that gets dropped -- kept, it is what the reference does.
// `hdr`/`radio` mirror CimbReader::update_metadata (CimbReader.cpp:269-280) when track_md is set.
__device__ __forceinline__ void aligner_block(FrameState& st, int block_no, int ok, const uint8_t* frame_chunks, bool track_md,
                                              uint8_t hdr[6], unsigned& radio)
{
	const int chunk_index = block_no / BLOCKS_PER_CHUNK;
	if (!ok) { st.bad = 1; st.offset = (st.offset + RS_DATA) % CHUNK; return; }
	if (RS_DATA + st.offset >= (unsigned)CHUNK) {
		const bool delivered = !st.bad;
		if (st.bad) { st.bad = 0; st.offset = 0; }
		else { st.mask |= 1u << chunk_index; st.offset = 0; }
		if (track_md) {
			if (!delivered && md_id(hdr) == 0) return;                       // update_metadata(nullptr, 0)
			if (md_id(hdr) == 0) { for (int k = 0; k < 6; ++k) hdr[k] = frame_chunks[(size_t)chunk_index * CHUNK + k]; }
			if (radio == 0) { unsigned fs = md_file_size(hdr); radio = (fs % CHUNK == 0) ? 0xFFFFFFFFu : fs / CHUNK; }
			md_increment(hdr, radio);
		}
		return;
	}
	st.offset += RS_DATA;
}

// Cell.h:30-62 mean_rgb_continuous(skip=false) over a 6x6 block whose top-left pixel is (x, y): uint16 sums / 36
__device__ __forceinline__ void mean6x6(const uint8_t* __restrict__ frame, int x, int y, uint32_t out[3])
{
	uint32_t r = 0, g = 0, b = 0;
#pragma unroll
	for (int i = 0; i < 6; ++i) {
		const uint8_t* p = frame + ((size_t)(y + i) * IMG_W + x) * 3;
#pragma unroll
		for (int j = 0; j < 6; ++j) { r += p[3 * j]; g += p[3 * j + 1]; b += p[3 * j + 2]; }
	}
	out[0] = (r & 0xFFFFu) / 36u; out[1] = (g & 0xFFFFu) / 36u; out[2] = (b & 0xFFFFu) / 36u;
}

// ---- float arithmetic that must match the CPU restatement operation for operation: no contraction, IEEE div/sqrt
#pragma clang fp contract(off)

// CimbReader.cpp:55-86 calculateWhite (dark): three 4x4 anchor-centre means (cv::mean -> double), max, floor (1,1,1).
// sums[a*3+c] = the integer sum of channel c over anchor a's 16 pixels; sum/16 is exact in double and in float.
__device__ __forceinline__ void white_from_sums(const uint32_t* sums, float white[3])
{
	white[0] = white[1] = white[2] = 1.0f;
	for (int a = 0; a < 3; ++a)
		for (int c = 0; c < 3; ++c) { float v = (float)((double)sums[a * 3 + c] / 16.0); if (v > white[c]) white[c] = v; }
}

// [assumed-OpenCV] lapack.cpp JacobiSVDImpl_<float>, n = 3 rows of length m = R (<= 5); same operation order as
// oracle/cimbar_oracle.c jacobi_svd_f32 (hypot spelled sqrt(p*p+beta*beta) in both)
// (m is a template constant -- 5 rows: four colours + white, the only shape init_ccm ever solves -- so that every array below lives in
// registers: with a runtime m the matrices sat in scratch memory and the kernel spent most of its 36 us waiting for it)
template <int m>
__device__ __forceinline__ void jacobi_svd3(float (&At)[3 * m], float (&Wout)[3], float (&Vt)[9])
{
	constexpr int n = 3;
	const double minval = FLT_MIN;
	const float eps = FLT_EPSILON * 2;
	double W[3];
	constexpr int max_iter = m > 30 ? m : 30;
#pragma unroll
	for (int i = 0; i < n; ++i) {
		double sd = 0;
#pragma unroll
		for (int k = 0; k < m; ++k) { float t = At[i * m + k]; sd += (double)t * t; }
		W[i] = sd;
#pragma unroll
		for (int k = 0; k < n; ++k) Vt[i * n + k] = 0;
		Vt[i * n + i] = 1;
	}
	for (int iter = 0; iter < max_iter; ++iter) {
		bool changed = false;
#pragma unroll
		for (int i = 0; i < n - 1; ++i)
#pragma unroll
			for (int j = i + 1; j < n; ++j) {
				float *Ai = &At[i * m], *Aj = &At[j * m];
				double a = W[i], p = 0, b = W[j];
#pragma unroll
				for (int k = 0; k < m; ++k) p += (double)Ai[k] * Aj[k];
				if (fabs(p) <= eps * sqrt(a * b)) continue;
				p *= 2;
				double beta = a - b, gamma = sqrt(p * p + beta * beta);
				float c, s;
				if (beta < 0) {
					double delta = (gamma - beta) * 0.5;
					s = (float)sqrt(delta / gamma);
					c = (float)(p / (gamma * s * 2));
				} else {
					c = (float)sqrt((gamma + beta) / (gamma * 2));
					s = (float)(p / (gamma * c * 2));
				}
				a = b = 0;
#pragma unroll
				for (int k = 0; k < m; ++k) {
					float t0 = c * Ai[k] + s * Aj[k];
					float t1 = -s * Ai[k] + c * Aj[k];
					Ai[k] = t0; Aj[k] = t1;
					a += (double)t0 * t0; b += (double)t1 * t1;
				}
				W[i] = a; W[j] = b;
				changed = true;
				float *Vi = &Vt[i * n], *Vj = &Vt[j * n];
#pragma unroll
				for (int k = 0; k < n; ++k) {
					float t0 = c * Vi[k] + s * Vj[k];
					float t1 = -s * Vi[k] + c * Vj[k];
					Vi[k] = t0; Vj[k] = t1;
				}
			}
		if (!changed) break;
	}
#pragma unroll
	for (int i = 0; i < n; ++i) {
		double sd = 0;
#pragma unroll
		for (int k = 0; k < m; ++k) { float t = At[i * m + k]; sd += (double)t * t; }
		W[i] = sqrt(sd);
	}
	// selection sort of three rows by singular value, descending: the same swaps, written as compile-time row pairs
#pragma unroll
	for (int i = 0; i < n - 1; ++i) {
		// j = index of the largest W among i..n-1 (first maximum, as `W[j] < W[k]` keeps the earlier one on ties)
#pragma unroll
		for (int cand = n - 1; cand > i; --cand) {
			bool is_j = true;
#pragma unroll
			for (int k = i; k < n; ++k) {
				if (k < cand) is_j = is_j && (W[k] < W[cand]);       // every earlier entry strictly smaller
				if (k > cand) is_j = is_j && !(W[cand] < W[k]);      // no later entry strictly larger
			}
			if (is_j) {
				double tw = W[i]; W[i] = W[cand]; W[cand] = tw;
#pragma unroll
				for (int k = 0; k < m; ++k) { float t = At[i * m + k]; At[i * m + k] = At[cand * m + k]; At[cand * m + k] = t; }
#pragma unroll
				for (int k = 0; k < n; ++k) { float t = Vt[i * n + k]; Vt[i * n + k] = Vt[cand * n + k]; Vt[cand * n + k] = t; }
				break;
			}
		}
	}
#pragma unroll
	for (int i = 0; i < n; ++i) Wout[i] = (float)W[i];
#pragma unroll
	for (int i = 0; i < n; ++i) {
		double sd = W[i];
		float s = (float)(sd > minval ? 1 / sd : 0.);
#pragma unroll
		for (int k = 0; k < m; ++k) At[i * m + k] *= s;
	}
}

// color_correction.h:26-39 get_moore_penrose_lsm: ccm = desired^T * pinv(actual^T) [assumed-OpenCV: SVD + SVBkSb + gemm]
template <int R>
__device__ __forceinline__ void moore_penrose_lsm(const float (&actual)[3 * R], const float (&desired)[3 * R], float (&ccm)[9])
{
	float A[3 * R], V[9], W[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
#pragma unroll
		for (int k = 0; k < R; ++k) A[i * R + k] = actual[k * 3 + i];
	jacobi_svd3<R>(A, W, V);
	float z[3 * R];
#pragma unroll
	for (int i = 0; i < R * 3; ++i) z[i] = 0;
	double threshold = 0;
#pragma unroll
	for (int i = 0; i < 3; ++i) threshold += W[i];
	threshold *= (double)(FLT_EPSILON * 2);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		double wi = W[k];
		if (fabs(wi) <= threshold) continue;
		wi = 1 / wi;
		double buffer[3];
#pragma unroll
		for (int j = 0; j < 3; ++j) buffer[j] = V[k * 3 + j] * wi;
#pragma unroll
		for (int i = 0; i < R; ++i) {
			float s = A[k * R + i];
#pragma unroll
			for (int j = 0; j < 3; ++j) z[i * 3 + j] = (float)(z[i * 3 + j] + s * buffer[j]);
		}
	}
#pragma unroll
	for (int i = 0; i < 3; ++i)
#pragma unroll
		for (int j = 0; j < 3; ++j) {
			double sm = 0;
#pragma unroll
			for (int k = 0; k < R; ++k) sm += (double)desired[k * 3 + i] * (double)z[k * 3 + j];
			ccm[i * 3 + j] = (float)sm;
		}
}

// color_correction.h:11-24 get_adaptation_matrix<von_kries>(white, (255,255,255)) -- color_correction == 1
__device__ void von_kries_ccm(const float white[3], float out[9])
{
	const float T[9] = {0.4002400f, 0.7076000f, -0.0808100f, -0.2263000f, 1.1653200f, 0.0457000f, 0.0000000f, 0.0000000f, 0.9182200f};
	float m1[3], m2[3], d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ti[9], tmp[9];
	for (int i = 0; i < 3; ++i) {
		float s = 0; for (int k = 0; k < 3; ++k) s += T[i * 3 + k] * white[k]; m1[i] = s;
		float q = 0; for (int k = 0; k < 3; ++k) q += T[i * 3 + k] * 255.0f; m2[i] = q;
	}
	for (int i = 0; i < 3; ++i) d[i * 3 + i] = m2[i] / m1[i];
#define A_(i, j) T[(i) * 3 + (j)]
	float det = (float)(A_(0,0) * (A_(1,1) * A_(2,2) - A_(2,1) * A_(1,2)) - A_(0,1) * (A_(1,0) * A_(2,2) - A_(2,0) * A_(1,2)) +
	                    A_(0,2) * (A_(1,0) * A_(2,1) - A_(2,0) * A_(1,1)));
	det = 1 / det;
	ti[0] = (A_(1,1) * A_(2,2) - A_(1,2) * A_(2,1)) * det; ti[1] = (A_(0,2) * A_(2,1) - A_(0,1) * A_(2,2)) * det;
	ti[2] = (A_(0,1) * A_(1,2) - A_(0,2) * A_(1,1)) * det; ti[3] = (A_(1,2) * A_(2,0) - A_(1,0) * A_(2,2)) * det;
	ti[4] = (A_(0,0) * A_(2,2) - A_(0,2) * A_(2,0)) * det; ti[5] = (A_(0,2) * A_(1,0) - A_(0,0) * A_(1,2)) * det;
	ti[6] = (A_(1,0) * A_(2,1) - A_(1,1) * A_(2,0)) * det; ti[7] = (A_(0,1) * A_(2,0) - A_(0,0) * A_(2,1)) * det;
	ti[8] = (A_(0,0) * A_(1,1) - A_(0,1) * A_(1,0)) * det;
#undef A_
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { float s = 0; for (int k = 0; k < 3; ++k) s += ti[i * 3 + k] * d[k * 3 + j]; tmp[i * 3 + j] = s; }
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { float s = 0; for (int k = 0; k < 3; ++k) s += tmp[i * 3 + k] * T[k * 3 + j]; out[i * 3 + j] = s; }
}

// CimbDecoder.cpp:168-200 get_best_color (+ :27-55, color_correction.h:64-68)
__device__ __forceinline__ uint32_t fix_single_color(float c, float adjust_up, float down)
{
	c -= down;
	c *= adjust_up;
	if (c > (245 - down)) c = 255;
	if (c < 0) c = 0;
	return (uint32_t)c & 0xFFu;
}
// The class and, with MARGIN, the classifier's confidence in it: margin = (second-smallest) - (smallest) squared distance, 0 for a tie that
// the first-minimum rule decides. One body for both so that class and margin cannot drift apart; best_color below is the class-only instance
// (k_colors), the colour erasure retry (erasure.hip.inc) takes the margin as well.
struct ColorFit { uint32_t best, margin; };
template <bool MARGIN>
__device__ __forceinline__ ColorFit color_fit(float r, float g, float b, const float* m, bool active)
{
	if (active) {
		float s0 = 0, s1 = 0, s2 = 0;
		s0 += m[0] * r; s0 += m[1] * g; s0 += m[2] * b;
		s1 += m[3] * r; s1 += m[4] * g; s1 += m[5] * b;
		s2 += m[6] * r; s2 += m[7] * g; s2 += m[8] * b;
		r = s0; g = s1; b = s2;
	}
	float mx = r; if (g > mx) mx = g; if (b > mx) mx = b; if (1.0f > mx) mx = 1.0f;
	float mn = r; if (g < mn) mn = g; if (b < mn) mn = b; if (48.0f < mn) mn = 48.0f;
	if (mn >= mx) mn = 0;
	// the reference computes 255.0/(max-min) in double and narrows to float (CimbDecoder.cpp:180). With both operands
	// exactly representable in binary32, double rounding through binary64 (53 >= 2*24+2 bits) is innocuous for division,
	// so the correctly rounded binary32 quotient is the same number -- and costs a third of the fp64 divide here.
	float adjust = __fdiv_rn(255.0f, mx - mn);
	int c0 = (int)fix_single_color(r, adjust, mn), c1 = (int)fix_single_color(g, adjust, mn), c2 = (int)fix_single_color(b, adjust, mn);
	int rel0 = c0 - c1, rel1 = c1 - c2, rel2 = c2 - c0;
	// CimbDecoder.cpp:186-198: the palette entry i minimising |rel - q_i|^2, q_i = (p0-p1, p1-p2, p2-p0), first minimum wins.
	// For the mode-B palette every q_i is a signed permutation of (255, -255, 0): |q_i|^2 is the same for all four, so the
	// minimum of the distance is the maximum of rel . q_i (first maximum wins) -- four differences instead of four
	// three-term squared distances:  q_0 = (-255, 255, 0), q_1 = (-255, 0, 255), q_2 = (0, 255, -255), q_3 = (255, -255, 0)
	// (the palette of c_palette -- {0,255,0},{0,255,255},{255,255,0},{255,0,255} -- is baked into these four differences)
	// The legacy palette (getColor4_old: cyan, yellow, magenta, green) is the same four colours in another order: the same four terms, ranked
	// in that order.
	if constexpr (NCOLORS != 4) {
		// eight colours (getColor8_old): the |q_i| differ, so the distances themselves; the float compare of CimbDecoder.cpp:192-197 is exact
		// for values this small
		uint32_t best = 0, best_d = 0xFFFFFFFFu, second_d = 0xFFFFFFFFu;
#pragma unroll
		for (int i = 0; i < NCOLORS; ++i) {
			const int q0 = c_palette[i][0] - c_palette[i][1], q1 = c_palette[i][1] - c_palette[i][2], q2 = c_palette[i][2] - c_palette[i][0];
			const uint32_t d = (uint32_t)((rel0 - q0) * (rel0 - q0) + (rel1 - q1) * (rel1 - q1) + (rel2 - q2) * (rel2 - q2));
			if constexpr (MARGIN) second_d = d < best_d ? best_d : (d < second_d ? d : second_d);
			if (d < best_d) { best = (uint32_t)i; best_d = d; }
		}
		return ColorFit{best, MARGIN ? second_d - best_d : 0u};
	}
	const int g_ = rel1 - rel0, c_ = rel2 - rel0, y_ = rel1 - rel2, m_ = rel0 - rel1;   // green, cyan, yellow, magenta
	const int t0 = LEGACY ? c_ : g_, t1 = LEGACY ? y_ : c_, t2 = LEGACY ? m_ : y_, t3 = LEGACY ? g_ : m_;
	uint32_t best_fit = 0;
	int bt = t0;
	if (t1 > bt) { best_fit = 1; bt = t1; }
	if (t2 > bt) { best_fit = 2; bt = t2; }
	if (t3 > bt) { best_fit = 3; bt = t3; }
	uint32_t margin = 0;
	if constexpr (MARGIN) {
		// distance_i = |rel|^2 + |q|^2 - 2 * 255 * t_i, so second-smallest - smallest distance = 510 * (largest - second-largest term)
		const int lo01 = t0 < t1 ? t0 : t1, hi01 = t0 < t1 ? t1 : t0, lo23 = t2 < t3 ? t2 : t3, hi23 = t2 < t3 ? t3 : t2;
		const int second = hi01 > hi23 ? (lo01 > hi23 ? lo01 : hi23) : (lo23 > hi01 ? lo23 : hi01);
		margin = 510u * (uint32_t)(bt - second);
	}
	return ColorFit{best_fit, margin};
}
__device__ __forceinline__ uint32_t best_color(float r, float g, float b, const float* m, bool active) { return color_fit<false>(r, g, b, m, active).best; }
#pragma clang fp contract(fast)

// K4: one wavefront per frame, after the symbol RS pass. Runs the chunk bookkeeping for blocks 0..39, then
// CimbReader::init_ccm (CimbReader.cpp:169-267) for color_correction == 2, or the von Kries matrix for == 1.
// ccm_out[f] = {9 floats, valid}; valid == 0 means "keep whatever the thread had" (resolved in k_colors).
__global__ __launch_bounds__(64) void k_frame_mid(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                  const uint8_t* __restrict__ chunks, const uint8_t* __restrict__ rs_ok,
                                                  int color_correction, FrameState* __restrict__ states, float* __restrict__ ccm_out, int f0,
                                                  int plain)
{
	const int f = f0 + blockIdx.x, lane = threadIdx.x;
	const uint8_t* frame = rgb + (size_t)f * FRAME_RGB;
	const uint8_t* fc = chunks + (size_t)f * FRAME_BYTES;
	__shared__ uint8_t s_hdr[4][6];      // predicted header of colour chunk c (CimbReader.cpp:188-227)
	__shared__ int s_have_hdr;
	__shared__ uint32_t s_cnt[4], s_r[4], s_g[4], s_b[4], s_first[4];

	// Everything this kernel reads from global memory is requested here, before anything waits: the kernel is one wavefront
	// per frame running a long serial chain (aligner, Jacobi SVD), so every dependent round trip to HBM shows in its latency.
	//   RS flags -> ballot, chunk headers -> LDS, the 96 header-predicted cells' means, the 48 anchor pixels of calculateWhite
	__shared__ uint8_t s_chunk_hdr[SYM_CHUNKS * CHUNK];   // only bytes [j*625, j*625+6) are filled / read (aligner_block's indexing)
	__shared__ uint32_t s_white[9];               // [anchor][channel] sums over the 4x4 anchor centres
	// (legacy modes: no Reed-Solomon pass has run yet -- their one stream is decoded after the colours -- so there are no flags and no headers)
	const uint8_t okb = !LEGACY && lane < SYM_BLOCKS ? rs_ok[(size_t)f * ALL_BLOCKS + lane] : (uint8_t)0;
	const uint8_t hdrb = !LEGACY && lane < SYM_CHUNKS * 6 ? fc[(size_t)(lane / 6) * CHUNK + lane % 6] : (uint8_t)0;
	const bool need_cells = color_correction == 2, need_white = color_correction == 1 || color_correction == 2;
	uint32_t mv0 = 0, mv1 = 0, px[3] = {0, 0, 0};
	if (need_cells) {
		if (lane < NHDR_CELLS) mv0 = cellmean[(size_t)f * GRID_CELLS + tb.ccm_grid[lane]];
		if (64 + lane < NHDR_CELLS) mv1 = cellmean[(size_t)f * GRID_CELLS + tb.ccm_grid[64 + lane]];
	}
	if (need_white && lane < 48) {
		// CimbReader.cpp:55-86 calculateWhite (dark): three 4x4 anchor-centre blocks; lane = anchor * 16 + row * 4 + col
		const int tl = ANCHOR - 2, farx = IMG_W - ANCHOR - 2, fary = IMG_H - ANCHOR - 2;   // {tl, tl}, {tl, bottom}, {right, tl}
		const int a = lane >> 4, ax = a == 2 ? farx : tl, ay = a == 1 ? fary : tl;
		const uint8_t* p = frame + ((size_t)(ay + ((lane >> 2) & 3)) * IMG_W + (ax + (lane & 3))) * 3;
		px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
	}
	if (lane < 9) s_white[lane] = 0;
	const unsigned long long ok_bits = __ballot(okb != 0);
	if (lane < SYM_CHUNKS * 6) s_chunk_hdr[(lane / 6) * CHUNK + lane % 6] = hdrb;
	__syncthreads();
	if (need_white && lane < 48) { atomicAdd(&s_white[(lane >> 4) * 3], px[0]); atomicAdd(&s_white[(lane >> 4) * 3 + 1], px[1]); atomicAdd(&s_white[(lane >> 4) * 3 + 2], px[2]); }
	if (lane == 0) {
		FrameState st = {0, 0, 0, 0};
		uint8_t hdr[6] = {0, 0, 0, 0, 0, 0};
		unsigned radio = 0;
		if (!LEGACY) for (int b = 0; b < SYM_BLOCKS; ++b) aligner_block(st, b, (int)((ok_bits >> b) & 1ull), s_chunk_hdr, true, hdr, radio);
		states[f] = st;
		// Decoder::decode into a plain stream has no aligned_stream, so no fountain header ever reaches the reader (Decoder.h:163-169)
		s_have_hdr = !plain && md_id(hdr) != 0;
		for (int c = 0; c < NHDR; ++c) {
			for (int k = 0; k < 6; ++k) s_hdr[c][k] = hdr[k];
			md_increment(hdr, radio);
		}
	}
	if (lane < 4) { s_cnt[lane] = 0; s_r[lane] = 0; s_g[lane] = 0; s_b[lane] = 0; s_first[lane] = 0xFFFFFFFFu; }
	__syncthreads();

	float* out = ccm_out + (size_t)f * 10;
	if (color_correction == 1) {
		if (lane == 0) {
			float white[3], m[9];
			white_from_sums(s_white, white);
			von_kries_ccm(white, m);
			for (int k = 0; k < 9; ++k) out[k] = m[k];
			out[9] = 1.0f;
		}
		return;
	}
	if (color_correction != 2 || !s_have_hdr) {
		if (lane == 0) out[9] = 0.0f;
		return;
	}

	// 96 known-colour cells: colour-stream cells 3100*c + t, t < 24; expected colour = bits [2t, 2t+2) of header c. Their means
	// (undrifted grid position + 1, 6x6, CimbReader.cpp:216-217: exactly what K1 left in cellmean) were fetched at the top.
	for (int q = lane; q < NHDR_CELLS; q += 64) {
		const int c = q / 24, t = q % 24;
		const uint32_t expected = ((uint32_t)s_hdr[c][t >> 2] >> (6 - 2 * (t & 3))) & 3u;
		const uint32_t mv = q < 64 ? mv0 : mv1;
		atomicAdd(&s_cnt[expected], 1u);
		atomicAdd(&s_r[expected], mv & 0xFFu);
		atomicAdd(&s_g[expected], (mv >> 8) & 0xFFu);
		atomicAdd(&s_b[expected], (mv >> 16) & 0xFFu);
		atomicMin(&s_first[expected], (uint32_t)q);
	}
	__syncthreads();

	if (lane == 0) {
		// rows in std::unordered_map iteration order = reverse order of first appearance (libstdc++, SURVEY 7.4 Q4). All four colours must
		// have been seen (CimbReader.cpp:251-253), so the system always has 5 rows: four colours + white. Row r = the colour with the
		// r-th LATEST first appearance, picked with compile-time row indices so that the matrices stay in registers.
		float actual[15], desired[15];
		const uint32_t cnt[4] = {s_cnt[0], s_cnt[1], s_cnt[2], s_cnt[3]};
		if (cnt[0] == 0 || cnt[1] == 0 || cnt[2] == 0 || cnt[3] == 0) { out[9] = 0.0f; return; }
		const uint32_t fa[4] = {s_first[0], s_first[1], s_first[2], s_first[3]};
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			int rank = 0;                       // how many colours appeared first AFTER this one
#pragma unroll
			for (int o = 0; o < 4; ++o) rank += fa[o] > fa[c] ? 1 : 0;
			const float ar = (float)(s_r[c] / cnt[c]), ag = (float)(s_g[c] / cnt[c]), ab = (float)(s_b[c] / cnt[c]);
#pragma unroll
			for (int r = 0; r < 4; ++r)
				if (rank == r) {
					actual[r * 3] = ar; actual[r * 3 + 1] = ag; actual[r * 3 + 2] = ab;
					desired[r * 3] = (float)c_palette[c][0]; desired[r * 3 + 1] = (float)c_palette[c][1]; desired[r * 3 + 2] = (float)c_palette[c][2];
				}
		}
		float white[3], m[9];
		white_from_sums(s_white, white);
		actual[12] = white[0]; actual[13] = white[1]; actual[14] = white[2];
		desired[12] = desired[13] = desired[14] = 255.0f;
		moore_penrose_lsm<5>(actual, desired, m);
		for (int k = 0; k < 9; ++k) out[k] = m[k];
		out[9] = 1.0f;
	}
}

constexpr int K5_CELLS = 7;   // 7 * 256 = 1792 grid slots per workgroup -> 7 workgroups per frame
constexpr int K5_BLOCKS = (GRID_CELLS + 256 * K5_CELLS - 1) / (256 * K5_CELLS);
// K5: colour pass (Decoder.h:107-113; CimbReader.cpp:133-137; CimbDecoder.cpp:202-217). The matrix in force for frame
// f is the newest valid one among frames <= f of this batch, else the context's carried one (slot `carry`).
// The kernel is a handful of loads and ~75 vector instructions per cell, so what it costs is dependent round trips: everything it reads is
// requested at the top, in one go -- the frame's flag, the cells' colour means (walked in GRID order, where K1 left them: contiguous dwords,
// the cell index follows from the slot arithmetically -- no look-up of a slot table first), the probe for the newest matrix and, speculatively,
// the frame's own matrix (the one the probe finds whenever the frame carried a header, i.e. nearly always).
// CARRY_IN (the mode auto-detection, automode_mode.hip.inc): `carry` is [n][10], the matrix in force for each frame that has none of its own --
// the frame before it in the reference's order may be an attempt in another mode, so there is no probe over the batch.
template <bool CARRY_IN>
__global__ __launch_bounds__(256) void k_colors(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ cellmean, Tables tb,
                                                const float* __restrict__ ccm_frames,
                                                const float* __restrict__ carry, const uint32_t* __restrict__ flood_flag,
                                                const int8_t* __restrict__ drift, uint8_t* __restrict__ colors,
                                                float* __restrict__ ccm_used, int f0)
{
	const int f = f0 + blockIdx.y;
	__shared__ float s_m[10];
	__shared__ int s_newest[4];
	const uint32_t flag = flood_flag[f];
	uint32_t mv[K5_CELLS];
	int ci[K5_CELLS];            // the slots' cells (tb.grid_cell: one coalesced 2-byte load per slot instead of ~20 instructions of band arithmetic, round 6)
#pragma unroll
	for (int k = 0; k < K5_CELLS; ++k) {
		const int g = (blockIdx.x * K5_CELLS + k) * 256 + threadIdx.x;
		mv[k] = g < GRID_CELLS ? cellmean[(size_t)f * GRID_CELLS + g] : 0u;
		ci[k] = g < GRID_CELLS ? (int)tb.grid_cell[g] : -1;
	}
	const float own = threadIdx.x < 10 ? ccm_frames[(size_t)f * 10 + threadIdx.x] : 0.0f;
	// newest frame g <= f of the batch that produced a matrix of its own: the workgroup probes 256 frames per round (thread t looks
	// at frame base - t), so a batch without any matrix costs n/256 rounds per workgroup instead of n dependent loads on one lane
	int g = -1;
	if constexpr (CARRY_IN) g = ccm_frames[(size_t)f * 10 + 9] != 0.0f ? f : -1;
	else for (int base = f; base >= 0 && g < 0; base -= 256) {
		const int cand = base - (int)threadIdx.x;
		const bool valid = cand >= 0 && ccm_frames[(size_t)cand * 10 + 9] != 0.0f;
		const unsigned long long m = __ballot(valid);
		if ((threadIdx.x & 63) == 0) s_newest[threadIdx.x >> 6] = m ? cand - (int)__builtin_ctzll(m) : -1;
		__syncthreads();
		for (int w = 3; w >= 0; --w) if (s_newest[w] >= 0) g = s_newest[w];   // wave 0 holds the newest frames
		__syncthreads();
	}
	if (threadIdx.x < 10) {
		const float v = g == f ? own : (g >= 0 ? ccm_frames[(size_t)g * 10 + threadIdx.x] : carry[(CARRY_IN ? (size_t)f * 10 : 0) + threadIdx.x]);
		s_m[threadIdx.x] = v;
		if (blockIdx.x == 0) ccm_used[(size_t)f * 10 + threadIdx.x] = v;
	}
	__syncthreads();
	const bool active = s_m[9] != 0.0f;
	const bool flooded = flag != 0;
#pragma unroll
	for (int k = 0; k < K5_CELLS; ++k) {
		const int i = ci[k];
		if (i < 0) continue;
		uint32_t col[3];
		if (flooded) {
			// the frame went through the exact flood pass: cells are read where their drift put them
			ushort2 xy = tb.cell_xy[i];
			const int x = (int)xy.x + drift[((size_t)f * NCELLS + i) * 2], y = (int)xy.y + drift[((size_t)f * NCELLS + i) * 2 + 1];
			mean6x6(rgb + (size_t)f * FRAME_RGB, x + 1, y + 1, col);
		} else {
			col[0] = mv[k] & 0xFFu; col[1] = (mv[k] >> 8) & 0xFFu; col[2] = (mv[k] >> 16) & 0xFFu;
		}
		colors[(size_t)f * NCELLS + i] = (uint8_t)best_color((float)col[0], (float)col[1], (float)col[2], s_m, active);
	}
}

// the matrix carried into the next call = the one in force for the batch's last frame (CimbDecoder.cpp:69-85). A kernel of its own
// for the split chain, where it must run after every part's colour pass has read the old carry.
__global__ __launch_bounds__(64) void k_carry_out(const float* __restrict__ ccm_used, float* __restrict__ carry, int f_last)
{
	if (threadIdx.x < 10) carry[threadIdx.x] = ccm_used[(size_t)f_last * 10 + threadIdx.x];
}

// K7: chunk bookkeeping for the colour blocks, final mask, zero the slots of dropped chunks, per-frame good bytes
__global__ __launch_bounds__(64) void k_frame_end(const uint8_t* __restrict__ rs_ok, FrameState* __restrict__ states,
                                                  uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks,
                                                  const float* __restrict__ ccm_used,
                                                  float* __restrict__ carry, int f0, int write_carry, int plain)
{
	const int f = f0 + blockIdx.x, lane = threadIdx.x;
	// the matrix carried into the next call = the one in force for the batch's last frame (CimbDecoder.cpp:69-85)
	if (write_carry && blockIdx.x == gridDim.x - 1 && lane < 10) carry[lane] = ccm_used[(size_t)f * 10 + lane];
	if (plain) {
		// Decoder::decode into a plain stream: every RS output is written where it falls, a failed block as 125 zero bytes
		// (reed_solomon_stream.h:62-74,96-107). masks[f] is not meaningful here; the per-block flags are in rs_ok.
		uint8_t* fb = chunks + (size_t)f * FRAME_BYTES;
		for (int b = 0; b < ALL_BLOCKS; ++b)
			if (!rs_ok[(size_t)f * ALL_BLOCKS + b])
				for (int k = lane; k < RS_DATA; k += 64) fb[(size_t)b * RS_DATA + k] = 0;
		if (lane == 0) masks[f] = 0;
		return;
	}
	__shared__ uint32_t s_mask;
	// the blocks this pass accounts for: the colour stream's (after k_frame_mid did the symbol stream's), or all of the legacy modes' one stream
	constexpr int NB = LEGACY ? ALL_BLOCKS : COL_BLOCKS, B0 = LEGACY ? 0 : SYM_BLOCKS;
	static_assert(NB <= 128, "block flags fit two ballots");
	const unsigned long long ok_bits = __ballot(lane < NB && rs_ok[(size_t)f * ALL_BLOCKS + B0 + (lane < NB ? lane : 0)] != 0);
	const unsigned long long ok_bits_hi = NB > 64 ? __ballot(64 + lane < NB && rs_ok[(size_t)f * ALL_BLOCKS + B0 + (64 + lane < NB ? 64 + lane : 0)] != 0) : 0ull;
	if (lane == 0) {
		FrameState st = states[f];
		uint8_t hdr[6] = {0, 0, 0, 0, 0, 0};
		unsigned radio = 0;
		for (int b = 0; b < NB; ++b) aligner_block(st, B0 + b, (int)(((b < 64 ? ok_bits : ok_bits_hi) >> (b & 63)) & 1ull), nullptr, false, hdr, radio);
		states[f] = st;
		masks[f] = st.mask;
		s_mask = st.mask;
	}
	__syncthreads();
	const uint32_t mask = s_mask;
	uint8_t* fc = chunks + (size_t)f * FRAME_BYTES;
	for (int j = 0; j < CHUNKS; ++j)
		if (!(mask & (1u << j)))
			for (int k = lane; k < CHUNK; k += 64) fc[(size_t)j * CHUNK + k] = 0;
}
