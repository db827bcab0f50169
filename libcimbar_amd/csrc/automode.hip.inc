// automode.hip.inc -- part of cimbar_hip.hip: mode auto-detection (cimbar_hip_auto_*, include/cimbar_hip.h). One batch of captures is tried in
// every candidate mode the way the reference's receiver tries them one after the other (web/recv.js:346,378: configure_decode + scan_extract_decode
// per mode until one returns bytes), with ONE colour-correction matrix carried across captures and modes, as the reference's thread_local one is
// (CimbDecoder.cpp:69-73; cimbard_configure_decode leaves it alone, cimbar_recv_js.cpp:272-288). DESIGN_WIDENING.md "Mode detection".
//
// An attempt = (capture f, candidate k). The symbol half of an attempt does not depend on the matrix, its colour half does. The scheme:
//   1. phase 0 = the first candidate's context scans every capture (the call's only scan), warps and runs the symbol half (automode_mode.hip.inc:
//      auto_symbols); k_auto_select appends the captures that delivered no symbol chunk to the next phase's list (one count per phase is read
//      back). Phase k > 0 gathers its captures dense (k_auto_gather) with their scan results (k_auto_scan_gather: NEEDS_SHARPEN judged for its
//      size), warps them into its geometry and runs the symbol half on them only
//   2. guess: each capture is accepted at its first candidate whose symbol half delivered (k_auto_guess)
//   3. k_auto_resolve walks the attempts in the reference's order under that guess and gives every attempt its matrix in force;
//      every phase's colour half runs with it (auto_colours)
//   4. k_auto_accept recomputes acceptance from the masks; where it differs from the guess, the new acceptances are adopted and 3-4 repeat.
//      Whether an attempt derives a matrix never depends on the matrix in force (color_correction 1: every attempt derives its own; 2: only
//      one with a fountain header, i.e. a symbol chunk, which is always accepted; 0: none), so the captures before the earliest change were
//      decoded with the right matrices, the earliest changed capture is settled after the round, and the loop ends within n + 1 rounds.
namespace {

constexpr int AUTO_MAX = 5;            // distinct modes of {68, 67, 66, 4, 8}

struct AutoPhases {                    // what the kernels need of the candidates of one call, in call order
	const float* ccm[AUTO_MAX];        // per phase: the matrices its frames derived ([n][10], k_frame_mid)
	float* carry_in[AUTO_MAX];         // per phase: the matrix in force for each frame without one of its own ([n][10], k_auto_resolve)
	const uint32_t* masks[AUTO_MAX];
	const uint8_t* chunks[AUTO_MAX];
	const int* status[AUTO_MAX];
	int status_stride[AUTO_MAX];
	int frame_bytes[AUTO_MAX], chunk[AUTO_MAX], mode[AUTO_MAX];
	int m[AUTO_MAX];                   // attempts of the phase (host side only)
};

// pos[k * n + f] = the slot of capture f in phase k's dense batch, -1 where it did not reach candidate k (row K: the captures that went past the last).
// first guess: the first candidate whose symbol half delivered a chunk (reached k, not k + 1, extraction fine); `first` = 1: every capture at its
// first candidate (CIMBAR_HIP_AUTO_GUESS_FIRST, a test switch: step 4 then has to repair the guess)
__global__ __launch_bounds__(256) void k_auto_guess(int K, int n, const int* __restrict__ pos, const int* __restrict__ status0, int stride0,
                                                    int first, int* __restrict__ acc)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= n) return;
	int a = K;
	if (first) a = 0;
	else if (status0[(size_t)f * stride0] > 0)
		for (int k = 0; k < K; ++k)
			if (pos[(size_t)k * n + f] >= 0 && pos[(size_t)(k + 1) * n + f] < 0) { a = k; break; }
	acc[f] = a;
}

// The matrix in force for every attempt under the acceptances acc[] (K = none): the reference's order is capture by capture, within a capture
// candidate by candidate up to the accepted one. An attempt uses the matrix of the newest attempt before it that derived one (k_frame_mid's
// valid flag), else the call's carry-in; a capture the extractor gave up on decodes in no mode and derives nothing (cimbar_recv_js.cpp:168-172).
// One workgroup of 1024 lanes: 1024 captures per round, the newest deriving attempt in front of each by a max-scan over (capture << 3 | candidate).
// carry_out = the matrix carried out of the call. Attempts after the accepted one get the matrix they would see had the capture gone on (every
// derivation of the capture's earlier attempts counted); only the accepted one's prefix is carried to the next capture.
__global__ __launch_bounds__(1024) void k_auto_resolve(int K, int n, const int* __restrict__ pos, const int* __restrict__ acc,
                                                       const int* __restrict__ status0, int stride0, AutoPhases P, const float* __restrict__ carry0,
                                                       float* __restrict__ carry_out)
{
	__shared__ int s_scan[1024];
	__shared__ float s_c0[10];
	__shared__ int s_run;
	const int t = threadIdx.x;
	if (t < 10) s_c0[t] = carry0[t];
	if (t == 0) s_run = -1;
	__syncthreads();
	auto matrix = [&](int key, int j) {      // element j of the matrix of attempt `key`, or of the call's carry-in
		if (key < 0) return s_c0[j];
		const int k = key & 7, g = key >> 3;
		return P.ccm[k][(size_t)pos[(size_t)k * n + g] * 10 + j];
	};
	for (int base = 0; base < n; base += 1024) {
		const int f = base + t;
		const bool ok = f < n && status0[(size_t)f * stride0] > 0;
		const int lim = ok ? (acc[f] < K ? acc[f] : K - 1) : -1;
		auto derived = [&](int k) { const int i = pos[(size_t)k * n + f]; return ok && i >= 0 && P.ccm[k][(size_t)i * 10 + 9] != 0.0f; };
		int ld = -1;
		for (int k = 0; k <= lim; ++k)
			if (derived(k)) ld = (f << 3) | k;
		s_scan[t] = ld;
		__syncthreads();
		for (int off = 1; off < 1024; off <<= 1) {
			const int v = t >= off ? s_scan[t - off] : -1;
			__syncthreads();
			if (v > s_scan[t]) s_scan[t] = v;
			__syncthreads();
		}
		int cur = t > 0 && s_scan[t - 1] > s_run ? s_scan[t - 1] : s_run;
		if (f < n)
			for (int k = 0; k < K; ++k) {
				const int i = pos[(size_t)k * n + f];
				if (i < 0) continue;
				float* dst = P.carry_in[k] + (size_t)i * 10;
				for (int j = 0; j < 10; ++j) dst[j] = matrix(cur, j);
				if (derived(k)) cur = (f << 3) | k;
			}
		__syncthreads();
		if (t == 0 && s_scan[1023] > s_run) s_run = s_scan[1023];
		__syncthreads();
	}
	if (t < 10) carry_out[t] = matrix(s_run, t);
}

// acceptance from the colour halves' masks: the first candidate the capture reached that delivered a chunk; *changed = 1 where that is not acc[f]
__global__ __launch_bounds__(256) void k_auto_accept(int K, int n, const int* __restrict__ pos, AutoPhases P, int* __restrict__ acc,
                                                     int* __restrict__ changed)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= n) return;
	int a = K;
	for (int k = 0; k < K; ++k) {
		const int i = pos[(size_t)k * n + f];
		if (i >= 0 && P.masks[k][i] != 0u) { a = k; break; }
	}
	if (a != acc[f]) { acc[f] = a; *changed = 1; }
}

// the caller's slots: the accepted attempt's chunks (zero-padded to the slot stride), mask, mode and extraction status; a capture no candidate
// delivered for: zeros, mode 0, the first candidate's status (the first phase is every capture, in batch order). *total += the good bytes.
__global__ __launch_bounds__(256) void k_auto_output(int K, int n, const int* __restrict__ pos, const int* __restrict__ acc, AutoPhases P, int slot,
                                                     uint8_t* __restrict__ chunks, uint32_t* __restrict__ masks, int* __restrict__ modes,
                                                     int* __restrict__ status, unsigned long long* __restrict__ total)
{
	const int f = blockIdx.x, k = acc[f];
	uint8_t* dst = chunks + (size_t)f * slot;
	if (k < K) {
		const int i = pos[(size_t)k * n + f];
		const uint8_t* src = P.chunks[k] + (size_t)i * P.frame_bytes[k];
		for (int b = threadIdx.x; b < slot; b += 256) dst[b] = b < P.frame_bytes[k] ? src[b] : (uint8_t)0;
		if (threadIdx.x == 0) {
			const uint32_t m = P.masks[k][i];
			masks[f] = m;
			modes[f] = P.mode[k];
			status[f] = P.status[k][(size_t)i * P.status_stride[k]];
			atomicAdd(total, (unsigned long long)__popc(m) * (unsigned long long)P.chunk[k]);
		}
	} else {
		for (int b = threadIdx.x; b < slot; b += 256) dst[b] = 0;
		if (threadIdx.x == 0) { masks[f] = 0; modes[f] = 0; status[f] = P.status[0][(size_t)f * P.status_stride[0]]; }
	}
}

// the first phase is every capture in batch order: pos[f] = f
__global__ __launch_bounds__(256) void k_auto_iota(int n, int* __restrict__ pos)
{
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f < n) pos[f] = f;
}

// a later phase's captures, dense: dst[i] = the capture list[i] of src (16-byte copies where the layout allows)
__global__ __launch_bounds__(256) void k_auto_gather(const uint8_t* __restrict__ src, size_t cbytes, const int* __restrict__ list, uint8_t* __restrict__ dst)
{
	const size_t i = blockIdx.y;
	const uint8_t* s = src + (size_t)list[i] * cbytes;
	uint8_t* d = dst + i * cbytes;
	const size_t step = (size_t)gridDim.x * 256 * 16;
	if ((((uintptr_t)s | (uintptr_t)d | cbytes) & 15) == 0) {
		for (size_t o = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16; o < cbytes; o += step)
			*reinterpret_cast<uint4*>(d + o) = *reinterpret_cast<const uint4*>(s + o);
	} else {
		for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < cbytes; o += step / 16) d[o] = s[o];
	}
}

#define AUTO_FWD(mode, c, fn, ...)                                                                   \
	((mode) == 67 ? m67::fn((m67::cimbar_hip_ctx*)(c), ##__VA_ARGS__)                                \
	 : (mode) == 66 ? m66::fn((m66::cimbar_hip_ctx*)(c), ##__VA_ARGS__)                              \
	 : (mode) == 4 ? m4::fn((m4::cimbar_hip_ctx*)(c), ##__VA_ARGS__)                                 \
	 : (mode) == 8 ? m8::fn((m8::cimbar_hip_ctx*)(c), ##__VA_ARGS__)                                 \
	               : m68::fn((m68::cimbar_hip_ctx*)(c), ##__VA_ARGS__))

}  // namespace

struct cimbar_hip_auto {
	int device = 0;
	int nmodes = 0;
	int modes[AUTO_MAX] = {};
	cimbar_hip_ctx* ctx[AUTO_MAX] = {};   // one context per candidate, in creation order
	int slot = 0;                         // cimbar_hip_auto_bufsize
	std::string err;
	Stream stream;
	DevBuf<float> d_carry;                // [10] the one carried matrix + [10] its value at the start of the call
	// per call, grown on demand
	int cap = 0;                          // captures the per-capture buffers below hold
	DevBuf<int> d_pos;                    // [K + 1][n]: slot of capture f in phase k's batch, -1 = did not reach it
	DevBuf<int> d_list;                   // [K + 1][n]: the captures of phase k's batch (row 0 unused: the first phase is every capture in order)
	DevBuf<uint8_t> d_dense;              // a later phase's captures, gathered
	DevBuf<int> d_acc;                    // [n] accepted candidate (K = none)
	DevBuf<int> d_small;                  // [AUTO_MAX] phase counts, [1] changed
	PinnedBuf<int> h_small;               // the same
	DevBuf<unsigned long long> d_total;
	PinnedBuf<unsigned long long> h_total;
	DevBuf<uint8_t> d_chunks[AUTO_MAX];   // per candidate: [n][its frame bytes]
	DevBuf<uint32_t> d_masks[AUTO_MAX];
	DevBuf<float> d_carry_in[AUTO_MAX];   // per candidate: [n][10]
	DevBuf<uint8_t> d_out;                // host-memory outputs: [n][slot] chunks, then masks, modes, status
	DevBuf<uint8_t> d_in;                 // host-memory captures

	// everything in flight is waited for, then the contexts go; the members free what is left
	~cimbar_hip_auto()
	{
		(void)hipSetDevice(device);
		(void)hipDeviceSynchronize();
		for (int k = 0; k < nmodes; ++k) if (ctx[k]) cimbar_hip_destroy(ctx[k]);
	}
};

namespace {

#define AUTOCHK(call)                                                                                     \
	do {                                                                                                  \
		hipError_t e__ = (call);                                                                          \
		if (e__ != hipSuccess) {                                                                          \
			a->err = std::string(#call) + ": " + hipGetErrorString(e__);                                  \
			return CIMBAR_HIP_EHIP;                                                                       \
		}                                                                                                 \
	} while (0)

int auto_capacity(cimbar_hip_auto* a, int n)
{
	if (n <= a->cap) return 0;
	AUTOCHK(hipDeviceSynchronize());
	a->cap = 0;
	const size_t N = (size_t)n;
	AUTOCHK(a->d_pos.reserve((AUTO_MAX + 1) * N));
	AUTOCHK(a->d_list.reserve((AUTO_MAX + 1) * N));
	AUTOCHK(a->d_acc.reserve(N));
	for (int k = 0; k < a->nmodes; ++k) {
		AUTOCHK(a->d_chunks[k].reserve(N * cimbar_hip_mode_bufsize(a->modes[k])));
		AUTOCHK(a->d_masks[k].reserve(N));
		AUTOCHK(a->d_carry_in[k].reserve(N * 10));
	}
	AUTOCHK(a->d_out.reserve((N * a->slot + 15) / 16 * 16 + N * 12));
	a->cap = n;
	return 0;
}

bool auto_mode_ok(int m) { return m == 68 || m == 67 || m == 66 || m == 4 || m == 8; }

}  // namespace

extern "C" {

int cimbar_hip_auto_create(int device, const int* modes, int n_modes, cimbar_hip_auto** out)
{
	if (!out) return CIMBAR_HIP_EINVAL;
	*out = nullptr;
	if (!modes || n_modes <= 0 || n_modes > AUTO_MAX) return CIMBAR_HIP_EINVAL;
	for (int i = 0; i < n_modes; ++i) {
		if (!auto_mode_ok(modes[i])) return CIMBAR_HIP_EINVAL;
		for (int j = 0; j < i; ++j) if (modes[j] == modes[i]) return CIMBAR_HIP_EINVAL;
	}
	cimbar_hip_auto* a = new cimbar_hip_auto;
	a->device = device;
	a->nmodes = n_modes;
	for (int i = 0; i < n_modes; ++i) {
		a->modes[i] = modes[i];
		const int b = cimbar_hip_mode_bufsize(modes[i]);
		if (b > a->slot) a->slot = b;
		if (int r = cimbar_hip_create(device, modes[i], &a->ctx[i])) { a->ctx[i] = nullptr; delete a; return r; }
	}
	auto fail = [&]() { delete a; return CIMBAR_HIP_EHIP; };
	if (hipSetDevice(device) != hipSuccess) return fail();
	if (a->stream.create() != hipSuccess) return fail();
	if (a->d_carry.reserve(20) != hipSuccess || hipMemset(a->d_carry, 0, sizeof(float) * 20) != hipSuccess) return fail();
	if (a->d_small.reserve(AUTO_MAX + 1) != hipSuccess || a->d_total.reserve(1) != hipSuccess) return fail();
	if (a->h_small.reserve(AUTO_MAX + 1) != hipSuccess || a->h_total.reserve(1) != hipSuccess) return fail();
	*out = a;
	return 0;
}

void cimbar_hip_auto_destroy(cimbar_hip_auto* a)
{
	delete a;
}

int cimbar_hip_auto_bufsize(const cimbar_hip_auto* a) { return a ? a->slot : CIMBAR_HIP_EINVAL; }

const char* cimbar_hip_auto_last_error(const cimbar_hip_auto* a) { return a ? a->err.c_str() : "null auto-detection object"; }

int cimbar_hip_auto_reset_ccm(cimbar_hip_auto* a)
{
	if (!a) return CIMBAR_HIP_EINVAL;
	AUTOCHK(hipSetDevice(a->device));
	AUTOCHK(hipDeviceSynchronize());
	AUTOCHK(hipMemset(a->d_carry, 0, sizeof(float) * 10));
	return 0;
}

int cimbar_hip_auto_get_ccm(cimbar_hip_auto* a, float out9[9])
{
	if (!a || !out9) return CIMBAR_HIP_EINVAL;
	float tmp[10];
	AUTOCHK(hipSetDevice(a->device));
	AUTOCHK(hipDeviceSynchronize());
	AUTOCHK(hipMemcpy(tmp, a->d_carry, sizeof tmp, hipMemcpyDeviceToHost));
	std::memcpy(out9, tmp, sizeof(float) * 9);
	return tmp[9] != 0.0f ? 1 : 0;
}

int cimbar_hip_auto_set_ccm(cimbar_hip_auto* a, const float m9[9])
{
	if (!a || !m9) return CIMBAR_HIP_EINVAL;
	float tmp[10];
	std::memcpy(tmp, m9, sizeof(float) * 9);
	tmp[9] = 1.0f;
	AUTOCHK(hipSetDevice(a->device));
	AUTOCHK(hipDeviceSynchronize());
	AUTOCHK(hipMemcpy(a->d_carry, tmp, sizeof tmp, hipMemcpyHostToDevice));
	return 0;
}

int64_t cimbar_hip_auto_scan_extract_decode_batch_fmt(cimbar_hip_auto* a, const int* order, int n_order, const uint8_t* img, unsigned width,
                                                      unsigned height, int format, int n, int img_mem, int preprocess, int color_correction,
                                                      uint8_t* chunks, uint32_t* masks, int* modes_out, int* status, int out_mem, void* hip_stream)
{
	if (!a) return CIMBAR_HIP_EINVAL;
	const char* who = "auto_scan_extract_decode_batch";
	if (!img || !chunks || !masks || !modes_out || !status || n <= 0 || width < 8 || height < 8) {
		a->err = std::string(who) + ": null buffer, n <= 0 or a capture smaller than 8x8";
		return CIMBAR_HIP_EINVAL;
	}
	if ((img_mem != CIMBAR_HIP_MEM_HOST && img_mem != CIMBAR_HIP_MEM_DEVICE) || (out_mem != CIMBAR_HIP_MEM_HOST && out_mem != CIMBAR_HIP_MEM_DEVICE)) {
		a->err = std::string(who) + ": img_mem / out_mem must be CIMBAR_HIP_MEM_HOST or CIMBAR_HIP_MEM_DEVICE";
		return CIMBAR_HIP_EINVAL;
	}
	// the candidates of this call: `order` picks (distinct) creation-time modes in the order they are tried
	int idx[AUTO_MAX], K = order ? n_order : a->nmodes;
	if (K <= 0 || K > a->nmodes) { a->err = std::string(who) + ": n_order must be 1 .. the number of modes the object was created with"; return CIMBAR_HIP_EINVAL; }
	for (int i = 0; i < K; ++i) {
		idx[i] = -1;
		for (int j = 0; j < a->nmodes; ++j) if (a->modes[j] == (order ? order[i] : a->modes[i])) idx[i] = j;
		bool dup = false;
		for (int j = 0; j < i; ++j) dup = dup || idx[j] == idx[i];
		if (idx[i] < 0 || dup) { a->err = std::string(who) + ": `order` must list distinct modes the object was created with"; return CIMBAR_HIP_EINVAL; }
	}
	const int fmt = m68::capture_format(format <= 0 ? 3 : format);
	if (!m68::capture_dims_ok(width, height, fmt)) { a->err = std::string(who) + m68::CAPTURE_DIMS_MSG; return CIMBAR_HIP_EDIM; }
	const size_t cbytes = cimbar_hip_capture_bytes(width, height, format <= 0 ? 3 : format);
	if ((uint64_t)width * height * 4 >= (1ull << 33) || cbytes >= ((size_t)1 << 31)) { a->err = std::string(who) + ": captures of 2 GiB or more are not supported"; return CIMBAR_HIP_EDIM; }
	// (the prologue of host.hip.inc's begin_call restated, not called: the object here is no mode's context -- its own error text and default
	// stream -- and nothing is drained here: each phase's auto_symbols waits for its own context's pipeline)
	AUTOCHK(hipSetDevice(a->device));
	const bool any_device = img_mem == CIMBAR_HIP_MEM_DEVICE || out_mem == CIMBAR_HIP_MEM_DEVICE;
	hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (any_device ? (hipStream_t)nullptr : a->stream);
	if (int r = auto_capacity(a, n)) return r;
	const uint8_t* d_in = img;
	if (img_mem == CIMBAR_HIP_MEM_HOST) {
		if (cbytes * n > a->d_in.capacity()) AUTOCHK(hipStreamSynchronize(st));   // (what an earlier call on this stream still reads is about to be replaced)
		AUTOCHK(a->d_in.reserve(cbytes * n));
		AUTOCHK(hipMemcpyAsync(a->d_in, img, cbytes * n, hipMemcpyHostToDevice, st));
		d_in = a->d_in;
	}
	AutoPhases P{};
	for (int k = 0; k < K; ++k) {
		const int j = idx[k], m = a->modes[j];
		P.carry_in[k] = a->d_carry_in[j];
		P.masks[k] = a->d_masks[j];
		P.chunks[k] = a->d_chunks[j];
		P.frame_bytes[k] = cimbar_hip_mode_bufsize(m);
		int32_t geo[CIMBAR_HIP_GEOMETRY_WORDS];
		cimbar_hip_geometry(a->ctx[j], geo);
		P.chunk[k] = geo[5];
		P.mode[k] = m;
	}
	const size_t N = (size_t)n;
	// 1. symbol halves, phase by phase: the first over every capture (it also runs the one scan of the call), each later one over the captures that
	//    reached it (gathered dense, the first phase's scan results gathered with them)
	AUTOCHK(hipMemsetAsync(a->d_pos, 0xFF, sizeof(int) * (size_t)(K + 1) * N, st));
	AUTOCHK(hipMemsetAsync(a->d_small, 0, sizeof(int) * (AUTO_MAX + 1), st));
	int ran = 0, m = n;
	const void* scan0 = nullptr;
	for (int k = 0; k < K; ++k) {
		int* list = a->d_list + (size_t)k * N;
		const uint8_t* d_phase = d_in;
		if (k > 0) {
			// how many captures reached this candidate: one small copy back per phase
			AUTOCHK(hipMemcpyAsync(a->h_small, a->d_small + (k - 1), sizeof(int), hipMemcpyDeviceToHost, st));
			AUTOCHK(hipStreamSynchronize(st));
			m = a->h_small[0];
			if (m == 0) break;
			AUTOCHK(a->d_dense.reserve(cbytes * m));
			hipLaunchKernelGGL(k_auto_gather, dim3(64, m), dim3(256), 0, st, d_in, cbytes, list, a->d_dense);
			d_phase = a->d_dense;
		}
		const int j = idx[k], md = a->modes[j];
		if (int r = AUTO_FWD(md, a->ctx[j], auto_symbols, st, d_phase, width, height, fmt, m, scan0, k > 0 ? list : nullptr, preprocess, color_correction,
		                     a->d_chunks[j], a->d_masks[j])) {
			a->err = std::string(who) + ": mode " + std::to_string(md) + ": " + cimbar_hip_last_error(a->ctx[j]);
			return r;
		}
		if (k == 0) {
			scan0 = AUTO_FWD(md, a->ctx[j], auto_scan_results);
			hipLaunchKernelGGL(k_auto_iota, dim3((n + 255) / 256), dim3(256), 0, st, n, a->d_pos);
		}
		if (int r = AUTO_FWD(md, a->ctx[j], auto_select, st, m, k > 0 ? list : nullptr, a->d_list + (size_t)(k + 1) * N, a->d_pos + (size_t)(k + 1) * N, a->d_small + k)) {
			a->err = std::string(who) + ": " + cimbar_hip_last_error(a->ctx[j]);
			return r;
		}
		P.m[k] = m;
		ran = k + 1;
	}
	// what the contexts hold of this call: read after the phases ran (a context allocates -- or grows -- its scratch in its first batch of this size)
	for (int k = 0; k < ran; ++k) {
		const int j = idx[k], md = a->modes[j];
		P.ccm[k] = AUTO_FWD(md, a->ctx[j], auto_ccm_frames);
		P.status[k] = AUTO_FWD(md, a->ctx[j], auto_status, &P.status_stride[k]);
	}
	// 2. the first guess
	static const int guess_first = [] { const char* v = std::getenv("CIMBAR_HIP_AUTO_GUESS_FIRST"); return v ? std::atoi(v) : 0; }();
	const dim3 g256((n + 255) / 256);
	hipLaunchKernelGGL(k_auto_guess, g256, dim3(256), 0, st, K, n, a->d_pos, P.status[0], P.status_stride[0], guess_first, a->d_acc);
	AUTOCHK(hipMemcpyAsync(a->d_carry + 10, a->d_carry, sizeof(float) * 10, hipMemcpyDeviceToDevice, st));
	// 3-4. matrices in force under the acceptances, colour halves, acceptance again -- until nothing changes
	for (int round = 0;; ++round) {
		if (round > n + 1) { a->err = std::string(who) + ": acceptance did not settle"; return CIMBAR_HIP_EHIP; }
		hipLaunchKernelGGL(k_auto_resolve, dim3(1), dim3(1024), 0, st, K, n, a->d_pos, a->d_acc, P.status[0], P.status_stride[0], P, a->d_carry + 10, a->d_carry);
		for (int k = 0; k < ran; ++k) {
			const int j = idx[k], md = a->modes[j];
			if (int r = AUTO_FWD(md, a->ctx[j], auto_colours, st, P.m[k], color_correction, a->d_carry_in[j], a->d_chunks[j], a->d_masks[j], round > 0)) {
				a->err = std::string(who) + ": " + cimbar_hip_last_error(a->ctx[j]);
				return r;
			}
		}
		AUTOCHK(hipMemsetAsync(a->d_small + AUTO_MAX, 0, sizeof(int), st));
		hipLaunchKernelGGL(k_auto_accept, g256, dim3(256), 0, st, K, n, a->d_pos, P, a->d_acc, a->d_small + AUTO_MAX);
		AUTOCHK(hipGetLastError());
		AUTOCHK(hipMemcpyAsync(a->h_small + AUTO_MAX, a->d_small + AUTO_MAX, sizeof(int), hipMemcpyDeviceToHost, st));
		AUTOCHK(hipStreamSynchronize(st));
		if (!a->h_small[AUTO_MAX]) break;
	}
	// 5. the caller's slots
	uint8_t* o_chunks = chunks; uint32_t* o_masks = masks; int* o_modes = modes_out; int* o_status = status;
	if (out_mem == CIMBAR_HIP_MEM_HOST) {
		o_chunks = a->d_out;
		o_masks = (uint32_t*)(a->d_out + (N * a->slot + 15) / 16 * 16);   // (8750-byte slots: the words after them start aligned)
		o_modes = (int*)(o_masks + N);
		o_status = o_modes + N;
	}
	AUTOCHK(hipMemsetAsync(a->d_total, 0, sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_auto_output, dim3(n), dim3(256), 0, st, K, n, a->d_pos, a->d_acc, P, a->slot, o_chunks, o_masks, o_modes, o_status, a->d_total);
	AUTOCHK(hipGetLastError());
	AUTOCHK(hipMemcpyAsync(a->h_total, a->d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	if (out_mem == CIMBAR_HIP_MEM_HOST) {
		AUTOCHK(hipMemcpyAsync(chunks, o_chunks, N * a->slot, hipMemcpyDeviceToHost, st));
		AUTOCHK(hipMemcpyAsync(masks, o_masks, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, st));
		AUTOCHK(hipMemcpyAsync(modes_out, o_modes, sizeof(int) * N, hipMemcpyDeviceToHost, st));
		AUTOCHK(hipMemcpyAsync(status, o_status, sizeof(int) * N, hipMemcpyDeviceToHost, st));
	}
	AUTOCHK(hipStreamSynchronize(st));
	return (int64_t)a->h_total[0];
}

}  // extern "C"
