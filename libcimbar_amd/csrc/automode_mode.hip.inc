// automode_mode.hip.inc -- part of mode.hip.inc (one copy per mode): what the mode auto-detection (automode.hip.inc) needs of one mode.
// An attempt = one capture decoded in one candidate mode. Phase k runs the attempts of candidate k as one dense batch of this mode's context --
// the captures that reached it, in the order of the phase's capture list -- in two halves: auto_symbols (warp + K1 + the symbol half of the chain,
// up to k_frame_mid) and auto_colours (the colour half, with the matrix in force supplied per frame, because the attempt before one in the
// reference's order may be an attempt in another mode).
namespace {

// a later phase's extraction results: dst[i] = src[list[i]] (the first phase's scan, which any mode's scan kernels compute alike: Extractor::extract
// reads the mode only through the size it warps to, Extractor.h:29-45), with NEEDS_SHARPEN judged again for this mode's size as k_scan_final does it
// (Corners::is_granular_scale, Corners.h:55-73)
__global__ __launch_bounds__(64) void k_auto_scan_gather(const ScanResult* __restrict__ src, const int* __restrict__ list, int m, ScanResult* __restrict__ dst)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i >= m) return;
	ScanResult r = src[list[i]];
	if (r.status > 0) {
		const int e[4][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}};
		bool granular = true;
		for (int k = 0; k < 4; ++k) {
			const int a = e[k][0], b = e[k][1];
			const int dx = abs((int)r.corners[2 * a] - (int)r.corners[2 * b]), dy = abs((int)r.corners[2 * a + 1] - (int)r.corners[2 * b + 1]);
			if (!(dx > IMG_W || dy > IMG_H)) granular = false;
		}
		r.status = granular ? 1 : 2;
	}
	dst[i] = r;
}

// after the symbol half of a phase: a capture goes on to the next candidate unless this attempt delivered a symbol chunk (then the reference's
// loop stops here whatever the colours do) or the extractor gave up on it (then every candidate's decode returns -3 and touches nothing).
// Legacy modes have no symbol stream of their own: their k_frame_mid leaves the mask empty, so every capture goes on. The captures that go on
// are appended to the next phase's list (one atomic per wavefront; lane order is kept inside a wavefront), pos_next[capture] = their slot.
__global__ __launch_bounds__(256) void k_auto_select(const FrameState* __restrict__ states, const int* __restrict__ status, int stride, int m,
                                                     const int* __restrict__ list, int* __restrict__ list_next, int* __restrict__ pos_next,
                                                     int* __restrict__ count)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const bool next = i < m && status[(size_t)i * stride] > 0 && states[i].mask == 0;
	const unsigned long long b = __ballot(next);
	const int lane = threadIdx.x & 63;
	int base = 0;
	if (lane == 0 && b) base = atomicAdd(count, (int)__popcll(b));
	base = __shfl(base, 0);
	if (next) {
		const int slot = base + (int)__popcll(b & ((1ull << lane) - 1ull));
		const int f = list ? list[i] : i;
		list_next[slot] = f;
		pos_next[f] = slot;
	}
}

}  // namespace

// the extraction status of the last auto_symbols batch: ints `*stride` apart
const int* auto_status(cimbar_hip_ctx* ctx, int* stride)
{
	*stride = (int)(sizeof(ScanResult) / sizeof(int));
	return &ctx->d_scan_res[0].status;
}
// ... its scan results (what a later phase's k_auto_scan_gather reads), and the matrix each of its frames derived ({9 floats, valid}, k_frame_mid)
const void* auto_scan_results(cimbar_hip_ctx* ctx) { return ctx->d_scan_res.get(); }
const float* auto_ccm_frames(cimbar_hip_ctx* ctx) { return ctx->cur().d_ccm_frames; }

// One phase's symbol half for m device-resident captures (dense: capture i of the phase at d_in + i * capture bytes). src_scan == nullptr: the
// first phase, which scans them itself; else the first phase's scan results, src_scan[list[i]] for capture i. Symbol chunks into d_chunks.
int auto_symbols(cimbar_hip_ctx* ctx, hipStream_t st, const uint8_t* d_in, unsigned width, unsigned height, int fmt, int m, const void* src_scan,
                 const int* list, int preprocess, int cc, uint8_t* d_chunks, uint32_t* d_masks)
{
	// (not begin_call: the stream and the mem flags are the auto context's business, automode.hip.inc)
	HIPCHK(hipSetDevice(ctx->device));
	if (int r = drain_pipeline_into(ctx, st)) return r;
	if (int r = ensure_capacity(ctx, m)) return r;
	// the capture front end with the anchor search swapped for a gather in the later phases (the captures are device-resident: nothing is staged)
	auto scan = [&](const uint8_t* d) -> int {
		if (!src_scan) return enqueue_scan(ctx, st, d, width, height, fmt, m);
		hipLaunchKernelGGL(k_auto_scan_gather, dim3((m + 63) / 64), dim3(64), 0, st, (const ScanResult*)src_scan, list, m, ctx->d_scan_res);
		hipLaunchKernelGGL(k_warp_matrices, dim3((m + 63) / 64), dim3(64), 0, st, ctx->d_scan_res[0].corners, sizeof(ScanResult) / sizeof(float),
		                   &ctx->d_scan_res[0].status, sizeof(ScanResult) / sizeof(int), m, ctx->d_ex_minv);
		return 0;
	};
	if (int r = capture_front(ctx, st, d_in, width, height, fmt, 0, m, CIMBAR_HIP_MEM_DEVICE, nullptr, nullptr, CIMBAR_HIP_MEM_DEVICE, scan)) return r;
	int stride;
	const int* status = auto_status(ctx, &stride);
	ChainArgs ca = chain_args(deskewed_source(ctx, status, stride, preprocess), m, cc, d_chunks, d_masks);   // (no_split: one chain on `st`)
	ca.symbols_only = true;                                   // the colour half is issued later, by auto_colours
	return enqueue(ctx, st, ca);
}

// the next phase's list from this one's m attempts (see k_auto_select); list == nullptr: this phase's list is 0 .. m-1
int auto_select(cimbar_hip_ctx* ctx, hipStream_t st, int m, const int* list, int* list_next, int* pos_next, int* count)
{
	int stride;
	const int* status = auto_status(ctx, &stride);
	hipLaunchKernelGGL(k_auto_select, dim3((m + 255) / 256), dim3(256), 0, st, ctx->cur().d_states, status, stride, m, list, list_next, pos_next, count);
	HIPCHK(hipGetLastError());
	return 0;
}

// the colour half of the last auto_symbols batch (m frames) with the matrix in force per frame (carry_in: [m][10]). again = true: a later round
// of the same batch -- the symbol RS pass and k_frame_mid run first once more (k_frame_end advances the frame's aligned_stream state and zeroes
// dropped chunk slots), so that the round gives what a first one with these matrices would have.
int auto_colours(cimbar_hip_ctx* ctx, hipStream_t st, int m, int cc, const float* d_carry_in, uint8_t* d_chunks, uint32_t* d_masks, bool again)
{
	cimbar_hip_ctx::ScratchSet& cur = ctx->cur();
	if (again) {
		if (!LEGACY) hipLaunchKernelGGL((k_rs<4>), dim3((m * SYM_BLOCKS + 3) / 4), dim3(256), 0, st, cur.d_symbols, ctx->tb, 0, m, 0, d_chunks, cur.d_rs_ok, 0);
		hipLaunchKernelGGL(k_frame_mid, dim3(m), dim3(64), 0, st, ctx->d_ex_frames, cur.d_cellmean, ctx->tb, d_chunks, cur.d_rs_ok, cc, cur.d_states, cur.d_ccm_frames, 0, 0);
	}
	hipLaunchKernelGGL((k_colors<true>), dim3(K5_BLOCKS, m), dim3(256), 0, st, ctx->d_ex_frames, cur.d_cellmean, ctx->tb, cur.d_ccm_frames, d_carry_in,
	                   cur.d_flood, cur.d_drift, cur.d_colors, cur.d_ccm_used, 0);
	if (LEGACY) hipLaunchKernelGGL((k_rs<(LEGACY ? CELL_BITS : 6)>), dim3((m * ALL_BLOCKS + 3) / 4), dim3(256), 0, st, cur.d_symbols, ctx->tb, 0, m, 0, d_chunks, cur.d_rs_ok, 0, cur.d_colors);
	else hipLaunchKernelGGL((k_rs<2>), dim3((m * COL_BLOCKS + 3) / 4), dim3(256), 0, st, cur.d_colors, ctx->tb, 0, m, SYM_CHUNKS, d_chunks, cur.d_rs_ok, SYM_BLOCKS);
	hipLaunchKernelGGL(k_frame_end, dim3(m), dim3(64), 0, st, cur.d_rs_ok, cur.d_states, d_chunks, d_masks, cur.d_ccm_used, ctx->d_carry, 0, 0, 0);
	int stride;
	const int* status = auto_status(ctx, &stride);
	hipLaunchKernelGGL(k_mask_failed, dim3(m), dim3(256), 0, st, status, stride, m, d_masks, d_chunks);
	HIPCHK(hipGetLastError());
	return 0;
}
