// extract.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace).
// X1-X4: the stage in front of the decoder (SURVEY 8(f) rank 2): Scanner's image preparation and Deskewer's perspective warp.
// ------------------------------------------------------------------------------------------------ extractor stage
// The reference hands a camera capture to Scanner (src/lib/extractor/Scanner.h:148-165: gray -> small Gaussian -> Otsu threshold,
// then a sparse scan-line search for the four anchors on the binary image, which stays on the host) and then to Deskewer::deskew
// (Deskewer.h:26-40: cv::getPerspectiveTransform + cv::warpPerspective INTER_LINEAR into the 1024x1024 frame the decoder wants).
// Both image passes are HBM-bound streaming / gather work over a 6 MB capture; the OpenCV arithmetic is restated exactly as in
// oracle/cimbar_oracle_extract.c [assumed-OpenCV: parity with a real OpenCV is unpinned, see DESIGN.md].

__device__ __forceinline__ int refl101(int i, int n)
{
	if (n == 1) return 0;
	while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
	return i;
}

// ---- capture formats: the `format` argument of the reference's C ABI (cimbard_scan_extract_decode, lib/cimbar_js/cimbar_recv_js.h:17) as
// get_rgb reads it (cimbar_recv_js.cpp:94-120): 12 = NV12 -> cvtColor(COLOR_YUV2RGB_NV12), 420 -> cvtColor(COLOR_YUV420p2RGB) -- which OpenCV
// defines as COLOR_YUV2RGB_YV12: the plane behind Y is read as V, the one after it as U --, 4 = RGBA -> cvtColor(COLOR_RGBA2RGB), anything
// else RGB8 as it is. The reference materialises the RGB image; here the two kernels that read a capture (X1 gray + blur, X4 warp) convert
// as they load, so a camera's 1.5 bytes per pixel are all that crosses PCIe and HBM.
// [assumed-OpenCV] color_yuv.simd.hpp, BT.601 in 20-bit fixed point: c = saturate_cast<uchar>((max(0, Y - 16) * CY + cuv) >> 20) with
//   ruv = 2^19 + CVR (V - 128), guv = 2^19 + CVG (V - 128) + CUG (U - 128), buv = 2^19 + CUB (U - 128); one (U, V) per 2x2 pixels.
constexpr int FMT_RGB = 3, FMT_RGBA = 4, FMT_NV12 = 12, FMT_I420 = 420;
// ---- the formats of native receivers (no reference front end takes them; each is defined by the cv::cvtColor code that makes the same RGB image):
//   21 = NV21 (Android): NV12 with the chroma pair stored (V, U) -> COLOR_YUV2RGB_NV21
//   422 = YUYV / YUY2, 4221 = UYVY (UVC webcams, capture cards; V4L2): 2 bytes per pixel, a row is w/2 groups (Y0, U, Y1, V) / (U, Y0, V, Y1); one
//     (U, V) pair serves the two pixels of its group and no other row -> COLOR_YUV2RGB_YUY2 / _UYVY. [assumed-OpenCV] color_yuv.simd.hpp runs 4:2:2
//     through the same uvToRGBuv / yRGBuvToRGBA as 4:2:0, so yuv_terms / yuv_rgb below are its arithmetic too
//   30 = BGR, 40 = BGRA (cv::VideoCapture, cv::imread) -> COLOR_BGR2RGB / COLOR_BGRA2RGB: a channel permutation
constexpr int FMT_NV21 = 21, FMT_YUYV = 422, FMT_UYVY = 4221, FMT_BGR = 30, FMT_BGRA = 40;
static_assert(FMT_RGB == CIMBAR_HIP_FMT_RGB && FMT_RGBA == CIMBAR_HIP_FMT_RGBA && FMT_NV12 == CIMBAR_HIP_FMT_NV12 && FMT_I420 == CIMBAR_HIP_FMT_I420 &&
              FMT_NV21 == CIMBAR_HIP_FMT_NV21 && FMT_YUYV == CIMBAR_HIP_FMT_YUYV && FMT_UYVY == CIMBAR_HIP_FMT_UYVY && FMT_BGR == CIMBAR_HIP_FMT_BGR &&
              FMT_BGRA == CIMBAR_HIP_FMT_BGRA, "the values named in cimbar_hip.h");
constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527, YUV_SHIFT = 20;
__host__ __device__ constexpr bool fmt_is_sp420(int f) { return f == FMT_NV12 || f == FMT_NV21; }            // Y plane + one plane of chroma pairs
__host__ __device__ constexpr bool fmt_is_420(int f) { return fmt_is_sp420(f) || f == FMT_I420; }
__host__ __device__ constexpr bool fmt_is_422(int f) { return f == FMT_YUYV || f == FMT_UYVY; }
__host__ __device__ constexpr bool fmt_is_bgr(int f) { return f == FMT_BGR || f == FMT_BGRA; }              // stored B, G, R(, A)
__host__ __device__ constexpr bool fmt_is_3byte(int f) { return f == FMT_RGB || f == FMT_BGR; }
__host__ __device__ constexpr bool fmt_is_4byte(int f) { return f == FMT_RGBA || f == FMT_BGRA; }
__host__ __device__ inline int capture_format(int f) { return (fmt_is_4byte(f) || fmt_is_420(f) || fmt_is_422(f) || f == FMT_BGR) ? f : FMT_RGB; }
__host__ __device__ inline size_t capture_bytes(size_t w, size_t h, int fmt)
{
	return fmt_is_420(fmt) ? w * h * 3 / 2 : w * h * (fmt_is_422(fmt) ? 2 : (fmt_is_4byte(fmt) ? 4 : 3));
}
// what a layout cannot hold: 4:2:0 an odd width or height, 4:2:2 an odd width (cv::cvtColor asserts)
inline bool capture_dims_ok(unsigned w, unsigned h, int fmt) { return !((fmt_is_420(fmt) && ((w | h) & 1u)) || (fmt_is_422(fmt) && (w & 1u))); }
constexpr const char* CAPTURE_DIMS_MSG = ": a 4:2:0 capture (format 12 / 21 / 420) needs an even width and height, a 4:2:2 capture (format 422 / 4221) an even width";
// one 4:2:2 group (two pixels, four bytes) as loaded: the lumas and the chroma pair
template <bool UYVY> __device__ __forceinline__ void yuv422_group(uint32_t g, uint32_t& y0, uint32_t& y1, uint32_t& u, uint32_t& v)
{
	if (UYVY) { u = g & 0xFFu; y0 = (g >> 8) & 0xFFu; v = (g >> 16) & 0xFFu; y1 = g >> 24; }
	else { y0 = g & 0xFFu; u = (g >> 8) & 0xFFu; y1 = (g >> 16) & 0xFFu; v = g >> 24; }
}
// B | G << 8 | R << 16 (| A << 24) -> R | G << 8 | B << 16: one v_perm_b32, the top byte cleared
__device__ __forceinline__ uint32_t swap_rb(uint32_t p) { return __builtin_amdgcn_perm(0u, p, 0x0C000102u); }
// the chroma terms of one (U, V) pair with the luma offset folded in: c = (max(Y, 16) * CY + k.c) >> 20, then saturate
struct YuvTerms { int r, g, b; };
__device__ __forceinline__ YuvTerms yuv_terms(uint32_t u, uint32_t v)
{
	const int uu = (int)u - 128, vv = (int)v - 128;
	constexpr int BASE = (1 << (YUV_SHIFT - 1)) - 16 * YUV_CY;
	YuvTerms k;
	k.r = BASE + __mul24(YUV_CVR, vv);
	k.g = BASE + __mul24(YUV_CVG, vv) + __mul24(YUV_CUG, uu);
	k.b = BASE + __mul24(YUV_CUB, uu);
	return k;
}
// R | G << 8 | B << 16
__device__ __forceinline__ uint32_t yuv_rgb(uint32_t Y, const YuvTerms& k)
{
	const int y = (int)(Y > 16u ? Y : 16u);
	const int r = (__mul24(y, YUV_CY) + k.r) >> YUV_SHIFT, g = (__mul24(y, YUV_CY) + k.g) >> YUV_SHIFT, b = (__mul24(y, YUV_CY) + k.b) >> YUV_SHIFT;
	const uint32_t R = (uint32_t)(r < 0 ? 0 : (r > 255 ? 255 : r)), G = (uint32_t)(g < 0 ? 0 : (g > 255 ? 255 : g)), B = (uint32_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
	return R | (G << 8) | (B << 16);
}
// A pixel is R | G << 8 | B << 16 and nothing above -- but the compiler builds the two low bytes of yuv_rgb's result with v_ashr_pk_u8_i32, shift +
// saturate + pack in one gfx950 instruction, and then ORs the result on as if its upper half were zero. It is not: in k_convert_roi R and G of every
// fourth pixel came out wrong. The kernels that read a pixel through byte selects never see it; code that shifts a pixel into its neighbour makes
// the value opaque and masks it, with this.
__device__ __forceinline__ uint32_t px_clean(uint32_t v) { asm volatile("" : "+v"(v)); return v & 0xFFFFFFu; }
// one pixel of a capture as R | G << 8 | B << 16, any format (the general path: borders, odd widths, the large blurs)
__device__ __forceinline__ uint32_t capture_px(const uint8_t* __restrict__ src, int sw, int sh, int fmt, int x, int y)
{
	if (fmt_is_3byte(fmt)) {
		const uint8_t* p = src + ((size_t)y * sw + x) * 3;
		const uint32_t c0 = p[0], c2 = p[2];
		return (fmt == FMT_BGR ? c2 : c0) | ((uint32_t)p[1] << 8) | ((fmt == FMT_BGR ? c0 : c2) << 16);
	}
	if (fmt_is_4byte(fmt)) { uint32_t v; __builtin_memcpy(&v, src + ((size_t)y * sw + x) * 4, 4); return fmt == FMT_BGRA ? swap_rb(v) : v & 0xFFFFFFu; }
	if (fmt_is_422(fmt)) {
		uint32_t g, y0, y1, u, v;
		__builtin_memcpy(&g, src + ((size_t)y * sw + (x & ~1)) * 2, 4);
		if (fmt == FMT_UYVY) yuv422_group<true>(g, y0, y1, u, v); else yuv422_group<false>(g, y0, y1, u, v);
		return yuv_rgb((x & 1) ? y1 : y0, yuv_terms(u, v));
	}
	const size_t plane = (size_t)sw * sh;
	const uint32_t Y = src[(size_t)y * sw + x];
	uint32_t u, v;
	if (fmt_is_sp420(fmt)) { const uint8_t* p = src + plane + (size_t)(y >> 1) * sw + (x & ~1); const int iu = fmt == FMT_NV21; u = p[iu]; v = p[iu ^ 1]; }
	else { const size_t ci = (size_t)(y >> 1) * (sw >> 1) + (x >> 1); v = src[plane + ci]; u = src[plane + (plane >> 2) + ci]; }
	return yuv_rgb(Y, yuv_terms(u, v));
}
// cvtColor(RGB2GRAY) of a packed pixel, left as gray16_T leaves it (gray = byte 2 of the result). BGR: the pixel as a B, G, R(, A) capture stores it
// -- the R and B weights change places in the constants, the instructions stay
template <bool BGR = false>
__device__ __forceinline__ uint32_t gray_T_of(uint32_t rgb)
{
	constexpr uint32_t LO2 = BGR ? 46u | (70u << 8) | (140u << 16) : 140u | (70u << 8) | (46u << 16);
	constexpr uint32_t HI = BGR ? 29u | (150u << 8) | (76u << 16) : 76u | (150u << 8) | (29u << 16);
	return (__builtin_amdgcn_udot4(rgb, HI, 0u, false) << 8) + __builtin_amdgcn_udot4(rgb, LO2, 32768u, false);
}

// X1: gray + R-radius Gaussian ([1 2 1]/4 or [1 4 6 4 1]/16, fixed point, one rounding, BORDER_REFLECT_101) + per-frame histogram.
// One workgroup per 128x32 output tile (X1_TILES of them, one below the other). The tile's RGB bytes (with the halo the blur needs) come in
// as aligned 16-byte loads -- every lane a full dwordx4, rows contiguous -- and are parked in LDS as they are; the gray tile is then built
// from LDS (reflection at the image border is an index computation there, not a per-pixel global gather), and every lane blurs 4 x 4
// outputs from dword reads of the gray tile. The first version loaded the capture a byte at a time and ran at 15 % of the HBM roofline.
constexpr int X1_TILES = 4, X1_TW = 128, X1_TH = 32;
// Gaussian weights (sum 2^s, s = 4 | 8 | 16 for the two passes together): the small fixed kernels of ksize 3 and 5, and for ksize 9
// getGaussianKernel(9, sigma <= 0): sigma = 1.7, 8.8 fixed point by getGaussianKernelFixedPoint_ED -> 4 13 30 51 60 51 30 13 4 [assumed-OpenCV]
// ksize 17 (captures of 4500 px and more on the short side): sigma = 2.9 -> 1 2 4 8 13 21 28 33 36 ... (oracle/cimbar_oracle_extract.c has the derivation)
template <int R> __device__ __forceinline__ constexpr int gauss_w(int i)
{
	constexpr int K17[9] = {1, 2, 4, 8, 13, 21, 28, 33, 36};
	return R == 1 ? (i == 1 ? 2 : 1) : R == 2 ? (i == 2 ? 6 : ((i == 1 || i == 3) ? 4 : 1))
	     : R == 4 ? (i == 4 ? 60 : ((i == 3 || i == 5) ? 51 : ((i == 2 || i == 6) ? 30 : ((i == 1 || i == 7) ? 13 : 4))))
	              : K17[i <= 8 ? i : 16 - i];
}
// RGB3: the capture is RGB8 and is staged as described above; otherwise (every other format, `fmt`) the gray tile is built pixel by
// pixel through capture_px -- this kernel is only the general path (odd widths, the 9x9 / 17x17 blurs), the streaming one below is the fast one.
template <int R, bool RGB3>
__global__ __launch_bounds__(256) void k_scan_gray_blur(const uint8_t* __restrict__ rgb, int w, int h, int fmt, uint8_t* __restrict__ out,
                                                        uint32_t* __restrict__ hist)
{
	constexpr int GW = X1_TW + 2 * R, GH = X1_TH + 2 * R, GSTRIDE = R == 8 ? 152 : 136, SHIFT = R == 1 ? 4 : (R == 2 ? 8 : 16);
	static_assert(R == 1 || R == 2 || R == 4 || R == 8, "ksize 3, 5, 9 or 17");
	constexpr int RAW_ROW = ((GW * 3 + 15 + 15) / 16) * 16;          // bytes of one staged row: the span plus up to 15 bytes of misalignment
	static_assert(GW <= GSTRIDE && GSTRIDE % 4 == 0, "gray rows are read as dwords");
	__shared__ __attribute__((aligned(16))) uint8_t s_raw[RGB3 ? GH : 1][RAW_ROW];
	__shared__ __attribute__((aligned(16))) uint8_t s_g[GH][GSTRIDE];
	// 16 interleaved copies of the histogram (copy = lane % 16, bin v of copy c at v * 16 + c): a capture is mostly flat background, so a
	// wavefront's 64 increments tend to hit ONE bin -- in one copy they would serialise, here they spread over 16 banks
	__shared__ uint32_t s_hist[256 * 16];
	const int f = blockIdx.z, x0 = blockIdx.x * X1_TW;
	const uint8_t* src = rgb + (size_t)f * capture_bytes((size_t)w, (size_t)h, RGB3 ? FMT_RGB : fmt);
	for (int k = threadIdx.x; k < 256 * 16; k += 256) s_hist[k] = 0;
	// columns staged per row: [xlo, xhi) = the tile +- R clipped to the image; reflected columns fall inside it
	const int xlo = max(0, x0 - R), xhi = min(w, x0 + X1_TW + R);
	for (int t = 0; t < X1_TILES; ++t) {
		const int y0 = (blockIdx.y * X1_TILES + t) * X1_TH;
		if (y0 >= h) break;
		__syncthreads();   // the previous tile's readers are done with the LDS
		// stage: row ty of the tile = image row refl101(y0 - R + ty); aligned 16-byte pieces from the one holding byte xlo*3 on
		if constexpr (RGB3)
		for (int ty = threadIdx.x >> 5; ty < GH; ty += 8) {
			const int gy = refl101(y0 - R + ty, h);
			const uint8_t* row = src + (size_t)gy * w * 3;
			const uintptr_t first = (uintptr_t)(row + (size_t)xlo * 3), base = first & ~(uintptr_t)15;
			const int nbytes = (int)(first - base) + (xhi - xlo) * 3, npieces = (nbytes + 15) / 16;
			const uintptr_t frame_end = (uintptr_t)(src + (size_t)w * h * 3);
			for (int c = threadIdx.x & 31; c < npieces; c += 32) {
				const uintptr_t addr = base + (uintptr_t)c * 16;
				uint4 v;
				if (addr + 16 <= frame_end) v = *reinterpret_cast<const uint4*>(addr);
				else {   // the last piece of the last frame: never read past the buffer
					uint8_t tmp[16];
					for (int k = 0; k < 16; ++k) tmp[k] = addr + k < frame_end ? *reinterpret_cast<const uint8_t*>(addr + k) : (uint8_t)0;
					v = *reinterpret_cast<const uint4*>(tmp);
				}
				*reinterpret_cast<uint4*>(&s_raw[ty][c * 16]) = v;
			}
		}
		if constexpr (RGB3) __syncthreads();
		// gray tile: tile column tx = image column refl101(x0 - R + tx)
		for (int idx = threadIdx.x; idx < GH * GW; idx += 256) {
			const int ty = idx / GW, tx = idx % GW;
			const int gy = refl101(y0 - R + ty, h);
			int gx = refl101(x0 - R + tx, w);
			gx = gx < xlo ? xlo : (gx >= xhi ? xhi - 1 : gx);   // (only columns right of the image, whose outputs are never stored, get clamped)
			if constexpr (RGB3) {
				const uint8_t* row = src + (size_t)gy * w * 3;
				const int off = (int)((uintptr_t)(row + (size_t)xlo * 3) & 15);
				const uint8_t* p = &s_raw[ty][off + (gx - xlo) * 3];
				s_g[ty][tx] = (uint8_t)((p[0] * 9798u + p[1] * 19235u + p[2] * 3735u + (1u << 14)) >> 15);   // cvtColor(RGB2GRAY)
			} else s_g[ty][tx] = (uint8_t)(gray_T_of(capture_px(src, w, h, fmt, gx, gy)) >> 16);
		}
		__syncthreads();
		// blur: lane -> 4 columns x 4 rows of outputs
		const int px = (threadIdx.x & 31) * 4, pyb = (threadIdx.x >> 5) * 4;
#pragma unroll
		for (int ry = 0; ry < 4; ++ry) {
			const int py = pyb + ry;
			const int x = x0 + px, y = y0 + py;
			int acc[4] = {0, 0, 0, 0};
#pragma unroll
			for (int a = 0; a <= 2 * R; ++a) {
				// tile bytes px .. px+3+2R = image columns x-R .. x+3+R, as dwords (px is a multiple of 4)
				constexpr int ND = (4 + 2 * R + 3) / 4;
				const uint32_t* dw = reinterpret_cast<const uint32_t*>(&s_g[py + a][px]);
				uint32_t bt[4 * ND];
#pragma unroll
				for (int q = 0; q < ND; ++q) {
					const uint32_t d = dw[q];
#pragma unroll
					for (int i = 0; i < 4; ++i) bt[4 * q + i] = (d >> (8 * i)) & 0xFFu;
				}
				const int ka = gauss_w<R>(a);
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					int rowv = 0;
#pragma unroll
					for (int j = 0; j <= 2 * R; ++j) rowv += gauss_w<R>(j) * (int)bt[k + j];
					acc[k] += ka * rowv;
				}
			}
			if (y < h && x < w) {
				uint32_t v[4], packed = 0;
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					v[k] = (uint32_t)(acc[k] + (1 << (SHIFT - 1))) >> SHIFT;
					packed |= v[k] << (8 * k);
					if (x + k < w) atomicAdd(&s_hist[v[k] * 16 + (threadIdx.x & 15)], 1u);
				}
				uint8_t* o = out + (size_t)f * w * h + (size_t)y * w + x;
				if (x + 3 < w && (w & 3) == 0) *reinterpret_cast<uint32_t*>(o) = packed;
				else
					for (int k = 0; k < 4 && x + k < w; ++k) o[k] = (uint8_t)v[k];
			}
		}
	}
	__syncthreads();
	uint32_t total = 0;
#pragma unroll
	for (int c = 0; c < 16; ++c) total += s_hist[threadIdx.x * 16 + ((c + threadIdx.x) & 15)];
	if (total) atomicAdd(&hist[(size_t)f * 256 + threadIdx.x], total);
}

// X1, streaming version for captures whose width is a multiple of 16 (every camera format; the tiled kernel above stays as the general path).
// Same shape as K1: no LDS staging, no workgroup barriers in the loop. One wavefront owns a strip of X1S_ROWS output rows of one column block;
// lane l holds the 16-pixel column group l-1 of the block (lanes 0 and lanes_out+1 are halo lanes: they compute gray for their neighbours
// and store nothing). Per row: three aligned dwordx4 loads per lane (rows DEPTH ahead already in flight), gray by v_dot4 (gray16_T), the
// horizontal pass on u16 pairs with the two neighbour pixels fetched by DPP wave shifts (BORDER_REFLECT_101 at the image's left / right
// edge = the lane's own pixels 1,2 / 14,13), a register ring of 2R+1 horizontally blurred rows for the vertical pass, one dwordx4 store.
// The largest intermediate is 256 * 255 < 2^16, so the whole blur stays in packed u16 arithmetic. Histogram: LDS atomics, 16 interleaved copies.
constexpr int X1S_ROWS = 30;
__device__ __forceinline__ void load48(const uint8_t* __restrict__ p, uint32_t d[12])
{
	const uint4* q = reinterpret_cast<const uint4*>(p);
	const uint4 a = q[0], b = q[1], c = q[2];
	d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
	d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
	d[8] = c.x; d[9] = c.y; d[10] = c.z; d[11] = c.w;
}
// One row of a capture as this lane's 16 pixels, per format: the dwords a lane keeps in flight (RowRegs<FMT>::N) and how they become the 16
// byte-aligned gray values gray16_T produces for RGB8.
//   RGB8  3 x dwordx4 (48 bytes)                        RGBA  4 x dwordx4; one v_dot4 pair per pixel, the alpha byte meets a zero coefficient
//   NV12  dwordx4 of Y + dwordx4 of the (U, V) row y/2  4:2:0 planes  dwordx4 of Y + dwordx2 from each chroma plane's row y/2
//   NV21  NV12's loads (the pair's bytes change places when it is taken apart)     BGR / BGRA  the RGB / RGBA loads (the weights change places)
//   YUYV / UYVY  2 x dwordx4: the lane's 16 pixels are 32 contiguous bytes, one dword = one chroma pair and its two lumas
// (widths are multiples of 16 and frames start 16-byte aligned on this path, so every one of those loads is naturally aligned: 4:2:2 rows are 2w
// and frames 2wh bytes, multiples of 32)
template <int FMT> struct RowRegs { static constexpr int N = fmt_is_3byte(FMT) ? 12 : (fmt_is_4byte(FMT) ? 16 : 8); };
template <int FMT>
__device__ __forceinline__ void capture_row_load(const uint8_t* __restrict__ frame, int w, int h, int y, int cl, uint32_t (&d)[RowRegs<FMT>::N])
{
	if constexpr (fmt_is_3byte(FMT)) load48(frame + ((size_t)y * w + (size_t)cl * 16) * 3, d);
	else if constexpr (fmt_is_4byte(FMT)) {
		const uint4* q = reinterpret_cast<const uint4*>(frame + ((size_t)y * w + (size_t)cl * 16) * 4);
#pragma unroll
		for (int k = 0; k < 4; ++k) { const uint4 a = q[k]; d[4 * k] = a.x; d[4 * k + 1] = a.y; d[4 * k + 2] = a.z; d[4 * k + 3] = a.w; }
	} else if constexpr (fmt_is_422(FMT)) {
		const uint4* q = reinterpret_cast<const uint4*>(frame + ((size_t)y * w + (size_t)cl * 16) * 2);
		const uint4 a = q[0], b = q[1];
		d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
		d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
	} else {
		const size_t plane = (size_t)w * h;
		const uint4 a = *reinterpret_cast<const uint4*>(frame + (size_t)y * w + (size_t)cl * 16);
		d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
		if constexpr (fmt_is_sp420(FMT)) {
			const uint4 c = *reinterpret_cast<const uint4*>(frame + plane + (size_t)(y >> 1) * w + (size_t)cl * 16);
			d[4] = c.x; d[5] = c.y; d[6] = c.z; d[7] = c.w;
		} else {
			const uint8_t* p1 = frame + plane + (size_t)(y >> 1) * (w >> 1) + (size_t)cl * 8;   // the plane behind Y: V, as COLOR_YUV420p2RGB reads it
			const uint2 v = *reinterpret_cast<const uint2*>(p1), u = *reinterpret_cast<const uint2*>(p1 + (plane >> 2));
			d[4] = v.x; d[5] = v.y; d[6] = u.x; d[7] = u.y;
		}
	}
}
template <int FMT>
__device__ __forceinline__ void capture_row_gray_T(const uint32_t (&d)[RowRegs<FMT>::N], uint32_t T[16])
{
	if constexpr (fmt_is_3byte(FMT)) gray_T<16, FMT == FMT_BGR>(d, T);
	else if constexpr (fmt_is_4byte(FMT)) {
#pragma unroll
		for (int p = 0; p < 16; ++p) T[p] = gray_T_of<FMT == FMT_BGRA>(d[p]);
	} else if constexpr (fmt_is_422(FMT)) {
#pragma unroll
		for (int c = 0; c < 8; ++c) {   // group c: pixels 2c, 2c+1 and their chroma pair in one dword
			uint32_t y0, y1, u, v;
			yuv422_group<FMT == FMT_UYVY>(d[c], y0, y1, u, v);
			const YuvTerms k = yuv_terms(u, v);
			T[2 * c] = gray_T_of(yuv_rgb(y0, k));
			T[2 * c + 1] = gray_T_of(yuv_rgb(y1, k));
		}
	} else {
#pragma unroll
		for (int c = 0; c < 8; ++c) {   // chroma sample c serves pixels 2c, 2c+1
			uint32_t u, v;
			if constexpr (fmt_is_sp420(FMT)) {
				const uint32_t uv = d[4 + (c >> 1)] >> (16 * (c & 1)), b0 = uv & 0xFFu, b1 = (uv >> 8) & 0xFFu;
				u = FMT == FMT_NV21 ? b1 : b0; v = FMT == FMT_NV21 ? b0 : b1;
			} else { v = (d[4 + (c >> 2)] >> (8 * (c & 3))) & 0xFFu; u = (d[6 + (c >> 2)] >> (8 * (c & 3))) & 0xFFu; }
			const YuvTerms k = yuv_terms(u, v);
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				const int p = 2 * c + q;
				T[p] = gray_T_of(yuv_rgb((d[p >> 2] >> (8 * (p & 3))) & 0xFFu, k));
			}
		}
	}
}

template <int R, int FMT>
__global__ __launch_bounds__(256) void k_scan_gray_blur_rows(const uint8_t* __restrict__ rgb, int w, int h, int lanes_out, uint8_t* __restrict__ out,
                                                             uint32_t* __restrict__ hist)
{
	constexpr int RN = 2 * R + 1, U = R == 1 ? 3 : 10, DEPTH = R == 1 ? 3 : 2, SHIFT = R == 1 ? 4 : 8;
	constexpr int NDW = RowRegs<FMT>::N;
	constexpr uint32_t HALF = (1u << (SHIFT - 1)) * 0x00010001u;
	static_assert(U % RN == 0 && U % DEPTH == 0, "ring and prefetch roles must be static after unrolling");
	__shared__ uint32_t s_hist[256 * 16];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int f = blockIdx.z;
	for (int k = threadIdx.x; k < 256 * 16; k += 256) s_hist[k] = 0;
	__syncthreads();
	const int ys = (blockIdx.y * 4 + wave) * X1S_ROWS;
	if (ys < h) {
		const int groups = w >> 4;
		const int c = blockIdx.x * lanes_out + lane - 1;               // this lane's 16-pixel column group
		const bool store = lane >= 1 && lane <= lanes_out && c < groups;
		const bool first = c == 0, last = c == groups - 1;
		const int cl = c < 0 ? 0 : (c >= groups ? groups - 1 : c);      // halo lanes outside the image load something valid; nobody uses it
		const uint8_t* src = rgb + (size_t)f * capture_bytes((size_t)w, (size_t)h, FMT);
		uint8_t* dst = out + (size_t)f * w * h + (size_t)cl * 16;
		const int rows = h - ys < X1S_ROWS ? h - ys : X1S_ROWS;
		const int total = rows + 2 * R;
		auto rowy = [&](int t) { return refl101(ys - R + (t < total ? t : total - 1), h); };
		uint32_t buf[DEPTH][NDW];
#pragma unroll
		for (int k = 0; k < DEPTH; ++k) capture_row_load<FMT>(src, w, h, rowy(k), cl, buf[k]);
		uint32_t ring[RN][8];
#pragma unroll
		for (int k = 0; k < RN; ++k)
#pragma unroll
			for (int i = 0; i < 8; ++i) ring[k][i] = 0;
		for (int t0 = 0; t0 < total; t0 += U) {
#pragma unroll
			for (int s = 0; s < U; ++s) {
				const int t = t0 + s;
				uint32_t (&d)[NDW] = buf[s % DEPTH];
				uint32_t T[16], G[8];
				capture_row_gray_T<FMT>(d, T);
				pairs_from_T(T, G);                                      // G[i] = pixel i | pixel i+8 << 16
				capture_row_load<FMT>(src, w, h, rowy(t + DEPTH), cl, d);
				// the pairs one and two pixels to the left / right of G[0] / G[7]
				const uint32_t l7 = from_left_lane(G[7], 0u), r0 = from_right_lane(G[0], 0u);
				const uint32_t pm1 = first ? (G[1] & 0xFFFFu) : (l7 >> 16), p16 = last ? (G[6] >> 16) : (r0 & 0xFFFFu);
				const uint32_t Gm1 = pm1 | (G[7] << 16), G8 = (G[0] >> 16) | (p16 << 16);
				uint32_t (&H)[8] = ring[s % RN];
				if (R == 1) {
#pragma unroll
					for (int i = 0; i < 8; ++i) H[i] = (i == 0 ? Gm1 : G[i - 1]) + 2u * G[i] + (i == 7 ? G8 : G[i + 1]);
				} else {
					const uint32_t l6 = from_left_lane(G[6], 0u), r1 = from_right_lane(G[1], 0u);
					const uint32_t pm2 = first ? (G[2] & 0xFFFFu) : (l6 >> 16), p17 = last ? (G[5] >> 16) : (r1 & 0xFFFFu);
					const uint32_t Gm2 = pm2 | (G[6] << 16), G9 = (G[1] >> 16) | (p17 << 16);
#pragma unroll
					for (int i = 0; i < 8; ++i) {
						const uint32_t a = i == 0 ? Gm2 : (i == 1 ? Gm1 : G[i - 2]), b = i == 0 ? Gm1 : G[i - 1];
						const uint32_t e = i == 7 ? G9 : (i == 6 ? G8 : G[i + 2]), dd = i == 7 ? G8 : G[i + 1];
						H[i] = a + 4u * b + 6u * G[i] + 4u * dd + e;
					}
				}
				if (t >= 2 * R && t < total) {
					const int yo = ys + t - 2 * R;
					uint32_t O[8];
#pragma unroll
					for (int i = 0; i < 8; ++i) {
						uint32_t v;
						if (R == 1) v = ring[(s + RN - 2) % RN][i] + 2u * ring[(s + RN - 1) % RN][i] + ring[s % RN][i];
						else v = ring[(s + RN - 4) % RN][i] + 4u * ring[(s + RN - 3) % RN][i] + 6u * ring[(s + RN - 2) % RN][i] + 4u * ring[(s + RN - 1) % RN][i] + ring[s % RN][i];
						O[i] = ((v + HALF) >> SHIFT) & 0x00FF00FFu;      // output pixel i | output pixel i+8 << 16
					}
					if (store) {
						const uint32_t t01 = __builtin_amdgcn_perm(O[1], O[0], 0x06020400u), t23 = __builtin_amdgcn_perm(O[3], O[2], 0x06020400u);
						const uint32_t t45 = __builtin_amdgcn_perm(O[5], O[4], 0x06020400u), t67 = __builtin_amdgcn_perm(O[7], O[6], 0x06020400u);
						uint4 o;
						o.x = __builtin_amdgcn_perm(t23, t01, 0x05040100u);   // pixels 0..3
						o.y = __builtin_amdgcn_perm(t67, t45, 0x05040100u);   // 4..7
						o.z = __builtin_amdgcn_perm(t23, t01, 0x07060302u);   // 8..11
						o.w = __builtin_amdgcn_perm(t67, t45, 0x07060302u);   // 12..15
						*reinterpret_cast<uint4*>(dst + (size_t)yo * w) = o;
						const uint32_t splat = (o.x & 0xFFu) * 0x01010101u;
						if (o.x == splat && o.y == splat && o.z == splat && o.w == splat) atomicAdd(&s_hist[(o.x & 0xFFu) * 16 + (lane & 15)], 16u);   // flat background
						else {
							const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
							for (int k = 0; k < 16; ++k) atomicAdd(&s_hist[((ow[k >> 2] >> (8 * (k & 3))) & 0xFFu) * 16 + (lane & 15)], 1u);
						}
					}
				}
			}
		}
	}
	__syncthreads();
	uint32_t total_bin = 0;
#pragma unroll
	for (int c = 0; c < 16; ++c) total_bin += s_hist[threadIdx.x * 16 + ((c + threadIdx.x) & 15)];
	if (total_bin) atomicAdd(&hist[(size_t)f * 256 + threadIdx.x], total_bin);
}

#pragma clang fp contract(off)
// X2: thresh.cpp getThreshVal_Otsu_8u, the double arithmetic in the reference order; one lane per frame
__global__ __launch_bounds__(64) void k_scan_otsu(const uint32_t* __restrict__ hist, int w, int h, int n, int* __restrict__ thr)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	const uint32_t* hs = hist + (size_t)f * 256;
	double mu = 0, scale = 1. / ((double)w * h);
	for (int i = 0; i < 256; ++i) mu += i * (double)hs[i];
	mu *= scale;
	double mu1 = 0, q1 = 0, max_sigma = 0;
	int max_val = 0;
	for (int i = 0; i < 256; ++i) {
		const double p_i = hs[i] * scale;
		mu1 *= q1;
		q1 += p_i;
		const double q2 = 1. - q1;
		if ((q1 < q2 ? q1 : q2) < (double)FLT_EPSILON || (q1 > q2 ? q1 : q2) > 1. - (double)FLT_EPSILON) continue;
		mu1 = (mu1 + i * p_i) / q1;
		const double mu2 = (mu - q1 * mu1) / q2;
		const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
		if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
	}
	thr[f] = max_val;
}

// X4: cv::warpPerspective(INTER_LINEAR, BORDER_CONSTANT 0) into a width x height RGB8 frame, four destination pixels per lane (their
// 12 bytes leave as three aligned dword stores). minv: the already inverted matrix (destination -> source), 9 doubles per frame.
// OpenCV evaluates the source position per 64-pixel block of a row as (X0 + M0*x1) with X0 taken at the block's left edge -- the same
// association is kept here, it decides the last bit. width must be a multiple of 4 (a lane's four pixels); it need not be one of 64: 1024 in
// modes 68 / 67 / 4 / 8, 736 in mode 66, whose twelfth 64-column tile is half empty (OpenCV's last block of a row is 32 wide there, with the same X0).
// FMT: the capture's pixel format. What cv::warpPerspective interpolates in the reference is the RGB image get_rgb made of the capture, so the
// four taps are converted (capture formats above) and then blended; nothing of that image exists in memory here.
// The two horizontally adjacent pixels (sx, sy), (sx + 1, sy) of an interior tap pair as R | G << 8 | B << 16 each:
template <int FMT>
__device__ __forceinline__ void capture_pair(const uint8_t* __restrict__ src, int sw, int sh, int sx, int sy, uint32_t& p0, uint32_t& p1)
{
	if constexpr (fmt_is_3byte(FMT)) {
		// six contiguous bytes: one 8-byte load (the caller keeps sx <= sw - 3, so it never leaves the frame). Offsets fit 32 bits (the host
		// refuses captures of 2^31 bytes or more). BGR / BGRA taps stay as stored: the blend is per channel, so remap_bilinear exchanges the
		// channels of its result, once per output pixel.
		uint2 r;
		__builtin_memcpy(&r, src + (uint32_t)(sy * sw + sx) * 3u, 8);
		p0 = r.x & 0xFFFFFFu;
		p1 = (r.x >> 24) | ((r.y & 0xFFFFu) << 8);
	} else if constexpr (fmt_is_4byte(FMT)) {
		uint2 r;
		__builtin_memcpy(&r, src + (size_t)(uint32_t)(sy * sw + sx) * 4u, 8);
		p0 = r.x & 0xFFFFFFu;
		p1 = r.y & 0xFFFFFFu;
	} else if constexpr (fmt_is_422(FMT)) {
		// the group of column sx & ~1 and the one after it: eight bytes of one row. sx even: both pixels in the first group (sx <= sw - 4, the width
		// being even: the second group is still inside the row); sx odd: the first group's second pixel and the second group's first, each with
		// its own chroma pair (2 sx + 6 <= 2 sw).
		uint2 g;
		__builtin_memcpy(&g, src + (uint32_t)(sy * sw + (sx & ~1)) * 2u, 8);
		uint32_t y0, y1, u, v, z0, z1, u1, v1;
		yuv422_group<FMT == FMT_UYVY>(g.x, y0, y1, u, v);
		yuv422_group<FMT == FMT_UYVY>(g.y, z0, z1, u1, v1);
		const YuvTerms k0 = yuv_terms(u, v), k1 = (sx & 1) ? yuv_terms(u1, v1) : k0;
		p0 = yuv_rgb((sx & 1) ? y1 : y0, k0);
		p1 = yuv_rgb((sx & 1) ? z0 : y1, k1);
	} else {
		const uint32_t plane = (uint32_t)sw * (uint32_t)sh;
		uint16_t yy;
		__builtin_memcpy(&yy, src + (uint32_t)(sy * sw + sx), 2);
		YuvTerms k0, k1;
		if constexpr (fmt_is_sp420(FMT)) {
			// the chroma pairs of columns sx & ~1 and (sx & ~1) + 2: four bytes (sx <= sw - 3 keeps them inside the row); NV12 stores (U, V), NV21 (V, U)
			uint32_t uv;
			__builtin_memcpy(&uv, src + plane + (uint32_t)((sy >> 1) * sw + (sx & ~1)), 4);
			if constexpr (FMT == FMT_NV21) uv = __builtin_amdgcn_perm(0u, uv, 0x02030001u);
			k0 = yuv_terms(uv & 0xFFu, (uv >> 8) & 0xFFu);
			k1 = (sx & 1) ? yuv_terms((uv >> 16) & 0xFFu, uv >> 24) : k0;
		} else {
			uint16_t vv, uu;
			const uint32_t ci = (uint32_t)((sy >> 1) * (sw >> 1) + (sx >> 1));
			__builtin_memcpy(&vv, src + plane + ci, 2);
			__builtin_memcpy(&uu, src + plane + (plane >> 2) + ci, 2);
			k0 = yuv_terms(uu & 0xFFu, vv & 0xFFu);
			k1 = (sx & 1) ? yuv_terms((uint32_t)uu >> 8, (uint32_t)vv >> 8) : k0;
		}
		p0 = yuv_rgb(yy & 0xFFu, k0);
		p1 = yuv_rgb((uint32_t)yy >> 8, k1);
	}
}
constexpr int WARP_ROWS = 4;
// Which tile of its frame a workgroup takes (round 6). The hardware deals consecutive workgroups round-robin to the eight XCDs, each with an L2 of its
// own, and a tile's 64 destination columns read ~183 source bytes per row -- 2.4 cache lines of 128 bytes for 1.4 lines' worth of pixels, the rest
// shared with the tiles to its left and right. In launch order (x fastest) those neighbours sit on OTHER XCDs and every shared line is fetched from
// HBM twice (profiles/r04zb: 10.7 GB fetched for 6.1 GB of source pixels, 77 % L2 misses). So the frame's tiles are dealt in eight contiguous runs:
// workgroup b of the frame (b = x + gridDim.x * y; its XCD is b % 8 when the tiles per frame are a multiple of eight) takes tile
// (b % 8) * (tiles / 8) + b / 8 -- one XCD walks a band of the frame left to right, row of tiles after row of tiles, and finds its neighbours' lines
// in its own L2. Shared by k_warp and k_undistort (undistort.hip.inc), whose gathers are near-identity as well.
__device__ __forceinline__ void xcd_tile(int xcd_order, int& bx, int& by)
{
	const unsigned tiles = gridDim.x * gridDim.y, b = blockIdx.x + gridDim.x * blockIdx.y;
	const unsigned t = (xcd_order && tiles % 8u == 0u) ? (b % 8u) * (tiles / 8u) + b / 8u : b;      // (xcd_order 0: launch order, CIMBAR_HIP_WARP_ORDER=0 -- for A/B runs)
	bx = (int)(t % gridDim.x); by = (int)(t / gridDim.x);
}
// remap's fixed-point INTER_LINEAR / BORDER_CONSTANT 0 tap (imgwarp.cpp remapBilinear) at the source position (X, Y) in 1/32 pixel, X = cvRound(32 x):
// one output pixel as R | G << 8 | B << 16, the source in capture format FMT converted as it is loaded. Shared by k_warp and k_undistort.
template <int FMT>
__device__ __forceinline__ uint32_t remap_bilinear(const uint8_t* __restrict__ src, int sw, int sh, int X, int Y)
{
	int sx = X >> 5, sy = Y >> 5;
	sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
	sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
	const int fx = X & 31, fy = Y & 31;
	uint32_t v = 0;
	if ((unsigned)sx < (unsigned)(sw - 2) && (unsigned)sy < (unsigned)(sh - 1)) {
		// all four taps inside the capture (every pixel but those on its border; column sw-2 goes the other way so that the wide loads of
		// capture_pair never leave the frame). The weights (32-fx)(32-fy)*32 ... factor,
		// sum = 32 * ((32-fy) * ((32-fx)*a0 + fx*a1) + fy * ((32-fx)*b0 + fx*b1)) exactly, so the reference's (sum + 2^14) >> 15 is (S + 512) >> 10.
		uint32_t a0p, a1p, b0p, b1p;
		capture_pair<FMT>(src, sw, sh, sx, sy, a0p, a1p);
		capture_pair<FMT>(src, sw, sh, sx, sy + 1, b0p, b1p);
		// per channel: the two taps of a row as bytes 0 / 1 of a dword (one v_perm_b32), times (32-fx, fx) with one v_dot4_u32_u8; the two row
		// sums (<= 8160) as the halves of a dword, times (32-fy, fy) with one v_dot2_u32_u16 that also adds the rounding term
		typedef unsigned short us2w __attribute__((ext_vector_type(2)));
		const uint32_t wx = (32u - (uint32_t)fx) | ((uint32_t)fx << 8);
		const us2w wy = us2w{(unsigned short)(32 - fy), (unsigned short)fy};
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const uint32_t sel = 0x0C0C0400u + (uint32_t)c * 0x0101u;       // byte 0 <- a0p[c], byte 1 <- a1p[c], bytes 2 / 3 <- 0
			const uint32_t ra = __builtin_amdgcn_udot4(__builtin_amdgcn_perm(a1p, a0p, sel), wx, 0u, false);
			const uint32_t rb = __builtin_amdgcn_udot4(__builtin_amdgcn_perm(b1p, b0p, sel), wx, 0u, false);
			const uint32_t S = __builtin_amdgcn_udot2(us2w{(unsigned short)ra, (unsigned short)rb}, wy, 512u, false);
			// (BGR / BGRA: the taps are as stored, channel c of them is channel 2 - c of the output -- the permutation commutes with the
			// per-channel blend, so it is this constant shift, once per output pixel, and not a v_perm per tap)
			v |= (S >> 10) << (8 * (fmt_is_bgr(FMT) ? 2 - c : c));
		}
	} else if (sx >= -1 && sx < sw && sy >= -1 && sy < sh) {   // border: taps outside read as 0 (BORDER_CONSTANT)
		const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
		const bool in_x0 = sx >= 0, in_x1 = sx + 1 < sw, in_y0 = sy >= 0, in_y1 = sy + 1 < sh;
		const uint32_t p00 = capture_px(src, sw, sh, FMT, in_x0 ? sx : 0, in_y0 ? sy : 0), p01 = capture_px(src, sw, sh, FMT, in_x1 ? sx + 1 : 0, in_y0 ? sy : 0);
		const uint32_t p10 = capture_px(src, sw, sh, FMT, in_x0 ? sx : 0, in_y1 ? sy + 1 : 0), p11 = capture_px(src, sw, sh, FMT, in_x1 ? sx + 1 : 0, in_y1 ? sy + 1 : 0);
		const int m00 = (in_y0 && in_x0) ? w00 : 0, m01 = (in_y0 && in_x1) ? w01 : 0, m10 = (in_y1 && in_x0) ? w10 : 0, m11 = (in_y1 && in_x1) ? w11 : 0;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const int s00 = (int)((p00 >> (8 * c)) & 0xFFu), s01 = (int)((p01 >> (8 * c)) & 0xFFu), s10 = (int)((p10 >> (8 * c)) & 0xFFu), s11 = (int)((p11 >> (8 * c)) & 0xFFu);
			v |= (uint32_t)(((s00 * m00 + s01 * m01 + s10 * m10 + s11 * m11) + (1 << 14)) >> 15) << (8 * c);
		}
	}
	return v;
}
template <int FMT>
__global__ __launch_bounds__(256) void k_warp(const uint8_t* __restrict__ rgb, int sw, int sh, const double* __restrict__ minv,
                                              uint8_t* __restrict__ out, int width, int height, int xcd_order)
{
	// A workgroup covers 64 columns x (16 x WARP_ROWS) rows, sixteen rows at a time: with one row group per workgroup the two million
	// short-lived workgroups of a 2 048-capture batch spent their time starting up (kernel arguments, the matrix, one dependent gather, done).
	// The tile order: xcd_tile above.
	int bx, by;
	xcd_tile(xcd_order, bx, by);
	const int f = blockIdx.z, xb = bx * 64, xq = (threadIdx.x & 15) * 4;
	if (xb + xq >= width) return;   // (width is a multiple of 4)
	const double* Mg = minv + (size_t)f * 9;
	const double M[9] = {Mg[0], Mg[1], Mg[2], Mg[3], Mg[4], Mg[5], Mg[6], Mg[7], Mg[8]};
	const uint8_t* src = rgb + (size_t)f * capture_bytes((size_t)sw, (size_t)sh, FMT);
#pragma unroll 1
	for (int it = 0; it < WARP_ROWS; ++it) {
	const int y = (by * WARP_ROWS + it) * 16 + (threadIdx.x >> 4);
	if (y >= height) break;
	const double X0 = M[0] * xb + M[1] * y + M[2];
	const double Y0 = M[3] * xb + M[4] * y + M[5];
	const double W0 = M[6] * xb + M[7] * y + M[8];
	uint32_t px[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int x1 = xq + k;
		double W = W0 + M[6] * x1;
		W = W != 0. ? 32. / W : 0.;
		double fX = (X0 + M[0] * x1) * W, fY = (Y0 + M[3] * x1) * W;
		fX = fX < (double)INT_MAX ? fX : (double)INT_MAX; fX = fX > (double)INT_MIN ? fX : (double)INT_MIN;
		fY = fY < (double)INT_MAX ? fY : (double)INT_MAX; fY = fY > (double)INT_MIN ? fY : (double)INT_MIN;
		const int X = (int)rint(fX), Y = (int)rint(fY);          // cvRound: round half to even
		px[k] = remap_bilinear<FMT>(src, sw, sh, X, Y);            // R | G << 8 | B << 16
	}
	uint32_t* o = reinterpret_cast<uint32_t*>(out + ((size_t)f * width * height + (size_t)y * width + xb + xq) * 3);
	o[0] = px[0] | (px[1] << 24);
	o[1] = (px[1] >> 8) | (px[2] << 16);
	o[2] = (px[2] >> 16) | (px[3] << 8);
	}
}
#pragma clang fp contract(fast)

// X4a (round 5): a YUV capture's RGB image, but only where the warp will look. What cv::warpPerspective interpolates in the reference is the RGB image
// get_rgb made of the capture (cimbar_recv_js.cpp:94-120); k_warp<12 | 420> converts a source pixel every time it is a tap -- four conversions per
// destination pixel. Here every source pixel inside the bounding box of the destination frame's pre-image is converted ONCE into a capture-shaped
// RGB8 scratch (same geometry, only the box is written), and k_warp<3> reads that. The box: the four corners of the destination frame through the
// inverted matrix (a projective map takes the square to a convex quadrilateral as long as the denominator keeps its sign: every tap lies inside the
// corners' bounding box), two pixels of margin for the fixed-point rounding and the +1 taps; any corner with a non-positive or non-finite denominator
// makes it the whole capture. One thread = 8 x 2 pixels (four 2x2 chroma blocks; in 4:2:2, where rows share no chroma, two rows of four groups).
// NV21 is NV12 with the pair's bytes exchanged on load.
// the box of one capture: {x0, y0, x1, y1} inclusive, or the whole capture (see above); one lane per capture
__global__ __launch_bounds__(64) void k_roi_boxes(const double* __restrict__ minv, int n, int sw, int sh, int width, int height, int4* __restrict__ boxes)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	const double* M = minv + (size_t)f * 9;
	int4 box = {0, 0, sw - 1, sh - 1};
	double lox = 1e300, loy = 1e300, hix = -1e300, hiy = -1e300;
	bool whole = false;
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const double x = (c & 1) ? (double)(width - 1) : 0.0, y = (c & 2) ? (double)(height - 1) : 0.0;
		const double W = M[6] * x + M[7] * y + M[8];
		if (!(W > 1e-12) || !(W < 1e300)) { whole = true; continue; }
		const double X = (M[0] * x + M[1] * y + M[2]) / W, Y = (M[3] * x + M[4] * y + M[5]) / W;
		if (!(X > -1e9 && X < 1e9 && Y > -1e9 && Y < 1e9)) { whole = true; continue; }
		lox = X < lox ? X : lox; hix = X > hix ? X : hix; loy = Y < loy ? Y : loy; hiy = Y > hiy ? Y : hiy;
	}
	if (!whole) {
		const int x0 = (int)floor(lox) - 2, x1 = (int)ceil(hix) + 3, y0 = (int)floor(loy) - 2, y1 = (int)ceil(hiy) + 3;
		box.x = x0 > 0 ? x0 : 0; box.y = y0 > 0 ? y0 : 0; box.z = x1 < sw - 1 ? x1 : sw - 1; box.w = y1 < sh - 1 ? y1 : sh - 1;
	}
	boxes[f] = box;
}

template <int FMT>
__global__ __launch_bounds__(256) void k_convert_roi(const uint8_t* __restrict__ cap, int sw, int sh, const int4* __restrict__ boxes, uint8_t* __restrict__ rgb_out)
{
	static_assert(fmt_is_420(FMT) || fmt_is_422(FMT), "only the YUV formats are converted ahead of the warp");
	const int f = blockIdx.z;
	const int4 box = boxes[f];
	const int bx0 = box.x, by0 = box.y, bx1 = box.z, by1 = box.w;
	// (a workgroup is 128 x 32 pixels: most of those outside the box leave here, on scalar compares)
	if ((int)blockIdx.x * 128 > bx1 || (int)blockIdx.x * 128 + 127 < bx0 || (int)blockIdx.y * 32 > by1 || (int)blockIdx.y * 32 + 31 < by0) return;
	const int x = (int)blockIdx.x * 128 + (int)(threadIdx.x & 15) * 8, y = (int)blockIdx.y * 32 + (int)(threadIdx.x >> 4) * 2;
	if (x >= sw || y >= sh || x + 7 < bx0 || x > bx1 || y + 1 < by0 || y > by1) return;
	const uint8_t* src = cap + (size_t)f * capture_bytes((size_t)sw, (size_t)sh, FMT);
	uint8_t* out = rgb_out + (size_t)f * ((size_t)sw * sh * 3);
	const size_t plane = (size_t)sw * sh;
	if ((sw & 7) == 0) {
		// the fast path (every camera size): 8 + 8 luma bytes and the 8 chroma bytes under them as aligned 8-byte (4:2:0 planes: 4-byte) loads, the two rows'
		// 24 RGB bytes each as three aligned 8-byte stores
		auto store_row = [&](int yy, const uint32_t (&p)[8]) {
			// eight pixels R | G << 8 | B << 16 -> 24 bytes
			uint2 a, bq, c;
			a.x = p[0] | (p[1] << 24); a.y = (p[1] >> 8) | (p[2] << 16);
			bq.x = (p[2] >> 16) | (p[3] << 8); bq.y = p[4] | (p[5] << 24);
			c.x = (p[5] >> 8) | (p[6] << 16); c.y = (p[6] >> 16) | (p[7] << 8);
			uint2* o = reinterpret_cast<uint2*>(out + ((size_t)yy * sw + x) * 3);
			o[0] = a; o[1] = bq; o[2] = c;
		};
		if constexpr (fmt_is_422(FMT)) {
			// 4:2:2: a row's eight pixels are four groups, 16 contiguous bytes; the two rows share nothing
#pragma unroll
			for (int r = 0; r < 2; ++r) {
				if (y + r >= sh) break;
				uint4 g;
				__builtin_memcpy(&g, src + ((size_t)(y + r) * sw + x) * 2, 16);
				const uint32_t gw[4] = {g.x, g.y, g.z, g.w};
				uint32_t px[8];
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					uint32_t y0, y1, u, v;
					yuv422_group<FMT == FMT_UYVY>(gw[q], y0, y1, u, v);
					const YuvTerms k = yuv_terms(u, v);
					px[2 * q] = px_clean(yuv_rgb(y0, k)); px[2 * q + 1] = px_clean(yuv_rgb(y1, k));
				}
				store_row(y + r, px);
			}
			return;
		}
		uint2 y0v, y1v;
		__builtin_memcpy(&y0v, src + (size_t)y * sw + x, 8);
		if (y + 1 < sh) __builtin_memcpy(&y1v, src + (size_t)(y + 1) * sw + x, 8); else y1v = y0v;
		uint32_t uu[4], vv[4];
		if constexpr (fmt_is_sp420(FMT)) {
			uint2 c;
			__builtin_memcpy(&c, src + plane + (size_t)(y >> 1) * sw + x, 8);
			if constexpr (FMT == FMT_NV21) { c.x = __builtin_amdgcn_perm(0u, c.x, 0x02030001u); c.y = __builtin_amdgcn_perm(0u, c.y, 0x02030001u); }   // (V, U) -> (U, V)
			uu[0] = c.x & 0xFFu; vv[0] = (c.x >> 8) & 0xFFu; uu[1] = (c.x >> 16) & 0xFFu; vv[1] = c.x >> 24;
			uu[2] = c.y & 0xFFu; vv[2] = (c.y >> 8) & 0xFFu; uu[3] = (c.y >> 16) & 0xFFu; vv[3] = c.y >> 24;
		} else {
			uint32_t cv, cu;
			const size_t ci = (size_t)(y >> 1) * (sw >> 1) + (x >> 1);
			__builtin_memcpy(&cv, src + plane + ci, 4);
			__builtin_memcpy(&cu, src + plane + (plane >> 2) + ci, 4);
#pragma unroll
			for (int q = 0; q < 4; ++q) { uu[q] = (cu >> (8 * q)) & 0xFFu; vv[q] = (cv >> (8 * q)) & 0xFFu; }
		}
		uint32_t px0[8], px1[8];
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const YuvTerms k = yuv_terms(uu[q], vv[q]);
			const uint32_t w0 = q < 2 ? y0v.x : y0v.y, w1 = q < 2 ? y1v.x : y1v.y;
			const int sft = 16 * (q & 1);
			px0[2 * q] = px_clean(yuv_rgb((w0 >> sft) & 0xFFu, k)); px0[2 * q + 1] = px_clean(yuv_rgb((w0 >> (sft + 8)) & 0xFFu, k));
			px1[2 * q] = px_clean(yuv_rgb((w1 >> sft) & 0xFFu, k)); px1[2 * q + 1] = px_clean(yuv_rgb((w1 >> (sft + 8)) & 0xFFu, k));
		}
		store_row(y, px0);
		if (y + 1 < sh) store_row(y + 1, px1);
		return;
	}
	const int npx = sw - x < 8 ? sw - x : 8;                       // (widths are even; a width that is no multiple of 8 ends inside a thread's run)
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const int xx = x + 2 * q;
		if (2 * q >= npx) break;
		uint32_t u = 0, v = 0;
		if constexpr (fmt_is_sp420(FMT)) { const uint8_t* p = src + plane + (size_t)(y >> 1) * sw + xx; u = p[FMT == FMT_NV21]; v = p[FMT != FMT_NV21]; }
		else if constexpr (FMT == FMT_I420) { const size_t ci = (size_t)(y >> 1) * (sw >> 1) + (xx >> 1); v = src[plane + ci]; u = src[plane + (plane >> 2) + ci]; }
		const YuvTerms k = yuv_terms(u, v);
#pragma unroll
		for (int r = 0; r < 2; ++r) {
			if (y + r >= sh) break;
			uint32_t p0, p1;
			if constexpr (fmt_is_422(FMT)) { p0 = capture_px(src, sw, sh, FMT, xx, y + r); p1 = capture_px(src, sw, sh, FMT, xx + 1, y + r); }
			else { const uint8_t* yr = src + (size_t)(y + r) * sw + xx; p0 = yuv_rgb(yr[0], k); p1 = yuv_rgb(yr[1], k); }
			uint8_t* o = out + ((size_t)(y + r) * sw + xx) * 3;
			o[0] = (uint8_t)p0; o[1] = (uint8_t)(p0 >> 8); o[2] = (uint8_t)(p0 >> 16);
			o[3] = (uint8_t)p1; o[4] = (uint8_t)(p1 >> 8); o[5] = (uint8_t)(p1 >> 16);
		}
	}
}

#pragma clang fp contract(off)
// cv::getPerspectiveTransform(corners, mode-B target points) as Deskewer::deskew calls it (Deskewer.h:28-36), then the 3x3 closed-form
// inverse cv::warpPerspective applies (no WARP_INVERSE_MAP): the destination -> source matrix the warp kernel wants. All in double, in
// OpenCV's operation order [assumed-OpenCV: LUImpl with partial pivoting; invert()'s n == 3 branch].
__host__ __device__ inline bool deskew_inverse_matrix(const float* src8, double Minv[9])
{
	const float sx = (float)IMG_W, sy = (float)IMG_H, anchor = (float)ANCHOR;   // Config::image_size_x/y(), Config::anchor_size(), padding 0
	const float dst8[8] = {anchor, anchor, sx - anchor, anchor, anchor, sy - anchor, sx - anchor, sy - anchor};
	double a[8][8], b[8];
	for (int i = 0; i < 4; ++i) {
		const float sx = src8[2 * i], sy = src8[2 * i + 1], dx = dst8[2 * i], dy = dst8[2 * i + 1];
		a[i][0] = a[i + 4][3] = sx;
		a[i][1] = a[i + 4][4] = sy;
		a[i][2] = a[i + 4][5] = 1;
		a[i][3] = a[i][4] = a[i][5] = a[i + 4][0] = a[i + 4][1] = a[i + 4][2] = 0;
		a[i][6] = -sx * dx; a[i][7] = -sy * dx;
		a[i + 4][6] = -sx * dy; a[i + 4][7] = -sy * dy;
		b[i] = dx; b[i + 4] = dy;
	}
	double* A = &a[0][0];
	const int m = 8;
	const double eps = DBL_EPSILON * 100;
	bool ok = true;
	for (int i = 0; i < m && ok; ++i) {
		int k = i;
		for (int j = i + 1; j < m; ++j) if (fabs(A[j * m + i]) > fabs(A[k * m + i])) k = j;
		if (fabs(A[k * m + i]) < eps) { ok = false; break; }
		if (k != i) { for (int j = i; j < m; ++j) { const double t = A[i * m + j]; A[i * m + j] = A[k * m + j]; A[k * m + j] = t; } const double t = b[i]; b[i] = b[k]; b[k] = t; }
		const double d = -1 / A[i * m + i];
		for (int j = i + 1; j < m; ++j) {
			const double alpha = A[j * m + i] * d;
			for (int c = i + 1; c < m; ++c) A[j * m + c] += alpha * A[i * m + c];
			b[j] += alpha * b[i];
		}
	}
	double S[9];
	if (ok)
		for (int i = m - 1; i >= 0; --i) {
			double s = b[i];
			for (int c = i + 1; c < m; ++c) s -= A[i * m + c] * b[c];
			b[i] = s / A[i * m + i];
		}
	for (int i = 0; i < 8; ++i) S[i] = ok ? b[i] : 0;
	S[8] = 1.;
	double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
	if (d == 0.) { for (int i = 0; i < 9; ++i) Minv[i] = 0; return false; }
	d = 1. / d;
	Minv[0] = (S[4] * S[8] - S[5] * S[7]) * d; Minv[1] = (S[2] * S[7] - S[1] * S[8]) * d; Minv[2] = (S[1] * S[5] - S[2] * S[4]) * d;
	Minv[3] = (S[5] * S[6] - S[3] * S[8]) * d; Minv[4] = (S[0] * S[8] - S[2] * S[6]) * d; Minv[5] = (S[2] * S[3] - S[0] * S[5]) * d;
	Minv[6] = (S[3] * S[7] - S[4] * S[6]) * d; Minv[7] = (S[1] * S[6] - S[0] * S[7]) * d; Minv[8] = (S[0] * S[4] - S[1] * S[3]) * d;
	return ok;
}
#pragma clang fp contract(fast)

// S3: the warp matrices of a batch straight from the scanner's corners (no host round trip); a capture whose search failed gets a matrix
// that maps every destination pixel outside the source: a black frame
struct ScanResult;
__global__ __launch_bounds__(64) void k_warp_matrices(const float* __restrict__ corners, size_t corner_stride_floats, const int* __restrict__ status,
                                                      size_t status_stride_ints, int n, double* __restrict__ minv)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	double M[9];
	const bool ok = !status || status[(size_t)f * status_stride_ints] > 0;
	if (ok) deskew_inverse_matrix(corners + (size_t)f * corner_stride_floats, M);
	// (failed search: a matrix that sends every destination pixel far outside the capture -> BORDER_CONSTANT black)
	const double far_away[9] = {0, 0, -1e6, 0, 0, -1e6, 0, 0, 1};
	for (int k = 0; k < 9; ++k) minv[(size_t)f * 9 + k] = ok ? M[k] : far_away[k];
}

// X3: out = v > t ? 255 : 0 in place, 16 bytes per lane
__global__ __launch_bounds__(256) void k_scan_binarize(uint8_t* __restrict__ img, size_t per_frame, const int* __restrict__ thr)
{
	const int f = blockIdx.y;
	const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
	if (i >= per_frame) return;
	const uint32_t t = (uint32_t)thr[f];
	uint8_t* p = img + (size_t)f * per_frame + i;
	if (i + 16 <= per_frame && (((uintptr_t)p) & 15) == 0) {
		uint4 v = *reinterpret_cast<uint4*>(p);
		uint32_t* q = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			uint32_t r = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b) r |= (((q[k] >> (8 * b)) & 0xFFu) > t ? 0xFFu : 0u) << (8 * b);
			q[k] = r;
		}
		*reinterpret_cast<uint4*>(p) = v;
	} else {
		for (int k = 0; k < 16 && i + k < per_frame; ++k) p[k] = p[k] > t ? 255 : 0;
	}
}
