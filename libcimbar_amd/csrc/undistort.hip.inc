// undistort.hip.inc -- part of cimbar_hip.hip (one translation unit; included inside its anonymous namespace, after extract.hip.inc and scan.hip.inc).
// U1-U2: the reference's lens undistortion in front of Extractor::extract (`cimbar --undistort`, exe/cimbar/cimbar.cpp:135-145):
// Undistort<SimpleCameraCalibration>::undistort (extractor/Undistort.h:11-62).
//   U1 k_undistort_calibrate  SimpleCameraCalibration::scan (SimpleCameraCalibration.h:30-58, SimpleCameraCalibration.cpp:1-75) after the anchor search
//                             of X1 + X2 + S1-S3 on the raw capture: Geometry::calculate_midpoints (Geometry.h:15-75), four Scanner::find_edge
//                             (Scanner.cpp:204-276, EdgeScanState.h), calculate_distortion_factor. One lane per capture: a few hundred pixel reads.
//   U2 k_undistort<FMT>       cv::initUndistortRectifyMap(camera, dist, Mat(), camera, size, CV_32FC1) and cv::remap(INTER_LINEAR, BORDER_CONSTANT)
//                             as one pass: the map is never materialised; every output pixel computes its own map entry in fp64 and gathers.
// Double arithmetic in the reference's operation order, no contraction (as k_scan_otsu and k4_frame.hip.inc), correctly rounded sqrt / division.
#pragma clang fp contract(off)

struct UdPt { double x, y; };
// point<double>::NONE() (Point.h): {inf, inf}
__device__ __forceinline__ UdPt ud_none() { return UdPt{__builtin_huge_val(), __builtin_huge_val()}; }
__device__ __forceinline__ bool ud_is_none(const UdPt& p) { return p.x == __builtin_huge_val() && p.y == __builtin_huge_val(); }

// Geometry::line_intersection (Geometry.h:17-38); false = NONE (|D| < 1e-8: parallel lines)
__device__ inline bool ud_line_intersection(UdPt a0, UdPt a1, UdPt b0, UdPt b1, UdPt& out)
{
	const double ax = a1.x - a0.x, ay = a0.y - a1.y, adet = a1.x * a0.y - a0.x * a1.y;
	const double bx = b1.x - b0.x, by = b0.y - b1.y, bdet = b1.x * b0.y - b0.x * b1.y;
	const double D = ay * bx - ax * by;
	if (fabs(D) < 1e-8) { out = ud_none(); return false; }
	const double Dx = adet * bx - ax * bdet;
	const double Dy = ay * bdet - adet * by;
	out = UdPt{__ddiv_rn(Dx, D), __ddiv_rn(Dy, D)};
	return true;
}

// Scanner::test_pixel (Scanner.cpp:52-59, dark mode) on the blurred gray plane of X1: `gray > Otsu threshold`. The reference's chase_edge reads
// pixels without a bounds check (undefined behaviour outside the image); here a tap whose truncated position leaves the plane is INACTIVE.
// (x, y) are the reference's doubles; the int conversion truncates as `int x = ...` / test_pixel(int, int) does.
struct UdPlane {
	const uint8_t* g; int w, h; uint32_t thr;
	__device__ __forceinline__ bool test(double x, double y) const
	{
		if (!(x > -1.0 && x < (double)w && y > -1.0 && y < (double)h)) return false;   // (NaN included)
		const int xi = (int)x, yi = (int)y;
		return g[(size_t)yi * w + xi] > thr;
	}
};

// Scanner::chase_edge (Scanner.cpp:212-224): 2 of the 4 points at -2, -1, 1, 2 units along `unit`
__device__ inline bool ud_chase_edge(const UdPlane& P, UdPt start, UdPt unit)
{
	int success = 0;
	const int steps[4] = {-2, -1, 1, 2};
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const double x = start.x + (unit.x * (double)steps[k]);
		const double y = start.y + (unit.y * (double)steps[k]);
		if (P.test(trunc(x), trunc(y))) ++success;
	}
	return success >= 2;
}

// Scanner::find_edge (Scanner.cpp:226-262): returns false for point<int>::NONE()
__device__ inline bool ud_find_edge(const UdPlane& P, int ux, int uy, int vx, int vy, UdPt mid, int& ex, int& ey)
{
	const UdPt dv{(double)vx - (double)ux, (double)vy - (double)uy};
	const UdPt dunit{__ddiv_rn(dv.x, 512.0), __ddiv_rn(dv.y, 512.0)};
	const UdPt out_v{__ddiv_rn(dv.y, 64.0), __ddiv_rn(dv.x, -64.0)};
	const UdPt in_v{-out_v.x, -out_v.y};
	if (ud_is_none(mid)) mid = UdPt{(double)ux + __ddiv_rn(dv.x, 2.0), (double)uy + __ddiv_rn(dv.y, 2.0)};
	const double adj = __ddiv_rn(30.0, 16.0);                      // _anchorSize / 16.0, _anchorSize = 30 (Scanner.h:183)
	mid.x += out_v.x * adj;
	mid.y += out_v.y * adj;
	for (int pass = 0; pass < 2; ++pass) {
		const UdPt check = pass == 0 ? out_v : in_v;
		// abs() here is the double overload (see DESIGN_WIDENING.md "Lens undistortion": the one real OpenCV's headers make visible)
		const double max_check = fmax(fabs(check.x), fabs(check.y));
		const UdPt unit{__ddiv_rn(check.x, max_check), __ddiv_rn(check.y, max_check)};
		// EdgeScanState: the length of a run of active pixels, reported at the first inactive pixel after it
		int state = 0, run = 0;
		double i = 0, j = 0;
		// (the loop runs at most 2 * max_check + 2 times: |dv| / 64 of a side of at most 65535 px)
		while (fabs(i) <= fabs(check.x) && fabs(j) <= fabs(check.y)) {
			const double x = mid.x + i;
			const double y = mid.y + j;
			if (x < 0 || x >= (double)P.w || y < 0 || y >= (double)P.h) {
				i += unit.x;
				j += unit.y;
				continue;
			}
			const bool active = P.test(x, y);
			int size = -1;
			if (state == 0) { if (active) { state = 1; run = 1; } }
			else if (active) ++run;
			else { state = 0; size = run; }
			if (size > 0) {
				const UdPt edge{x - __ddiv_rn(unit.x * (double)size, 2.0), y - __ddiv_rn(unit.y * (double)size, 2.0)};
				if (ud_chase_edge(P, edge, dunit)) { ex = (int)edge.x; ey = (int)edge.y; return true; }
			}
			i += unit.x;
			j += unit.y;
		}
	}
	return false;
}

// sqrt((double)a.squared_distance(b)) (SimpleCameraCalibration.cpp:8-12; Point.h squared_distance = pow(dx, 2) + pow(dy, 2), exact as dx * dx)
__device__ __forceinline__ double ud_distance(double ax, double ay, double bx, double by)
{
	const double dx = bx - ax, dy = by - ay;
	return __dsqrt_rn(dx * dx + dy * dy);
}

// SimpleCameraCalibration::scan per capture, after the anchor search: ok = 1 and k1 = calculate_distortion_factor where the reference returns
// parameters, ok = 0 (k1 = 0) where it returns {} (fewer than 4 anchors, or calculate_midpoints found parallel sides). target: _targetRatio.
__global__ __launch_bounds__(64) void k_undistort_calibrate(const uint8_t* __restrict__ gray, int w, int h, const int* __restrict__ thr,
                                                            const int* __restrict__ status, int status_stride, const float* __restrict__ corners,
                                                            int corner_stride, int n, double target, int* __restrict__ ok_out, double* __restrict__ k1_out)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	ok_out[f] = 0;
	k1_out[f] = 0.;
	if (status[(size_t)f * status_stride] <= 0) return;          // Scanner::scan found fewer than 4 anchors (or its lists overflowed): {}
	const float* c = corners + (size_t)f * corner_stride;        // Corners::all(): top-left, top-right, bottom-left, bottom-right
	const int tlx = (int)c[0], tly = (int)c[1], trx = (int)c[2], try_ = (int)c[3], blx = (int)c[4], bly = (int)c[5], brx = (int)c[6], bry = (int)c[7];
	const UdPt tl{(double)tlx, (double)tly}, tr{(double)trx, (double)try_}, bl{(double)blx, (double)bly}, br{(double)brx, (double)bry};
	// Geometry::calculate_midpoints
	UdPt center, lr_inf, tb_inf;
	if (!ud_line_intersection(tl, br, tr, bl, center)) return;
	if (!ud_line_intersection(tr, br, tl, bl, lr_inf)) return;
	if (!ud_line_intersection(tl, tr, bl, br, tb_inf)) return;
	UdPt mid[4];
	ud_line_intersection(tl, tr, center, lr_inf, mid[0]);        // top    (NONE stays NONE: find_edge then takes the side's middle)
	ud_line_intersection(tr, br, center, tb_inf, mid[1]);        // right
	ud_line_intersection(bl, br, center, lr_inf, mid[2]);        // bottom
	ud_line_intersection(tl, bl, center, tb_inf, mid[3]);        // left
	// Scanner::scan_edges: top (tl -> tr), right (tr -> br), bottom (br -> bl), left (bl -> tl)
	const UdPlane P{gray + (size_t)f * w * h, w, h, (uint32_t)thr[f]};
	const int su[4][2] = {{tlx, tly}, {trx, try_}, {brx, bry}, {blx, bly}}, sv[4][2] = {{trx, try_}, {brx, bry}, {blx, bly}, {tlx, tly}};
	double ratios[4];
	int nr = 0;
	for (int e = 0; e < 4; ++e) {
		int ex, ey;
		if (!ud_find_edge(P, su[e][0], su[e][1], sv[e][0], sv[e][1], mid[e], ex, ey)) continue;
		// get_distortion_factor: distance(observed, expected) / distance(start, end)
		const double num = ud_distance((double)ex, (double)ey, mid[e].x, mid[e].y);
		const int dx = sv[e][0] - su[e][0], dy = sv[e][1] - su[e][1];
		const double den = __dsqrt_rn((double)(dx * dx + dy * dy));
		ratios[nr++] = __ddiv_rn(num, den);
	}
	double k1 = 0.;                                              // no ratio at all: `return {}` -- 0, and still a success
	if (nr > 0) {
		double total = 0;
		for (int k = 0; k < nr; ++k) total += ratios[k];
		double smallest = target - __ddiv_rn(total, (double)nr);
		for (int k = 0; k < nr; ++k) {
			const double dist = target - ratios[k];
			if (fabs(dist) < fabs(smallest)) smallest = dist;
		}
		k1 = smallest;
	}
	ok_out[f] = 1;
	k1_out[f] = k1;
}

// The per-batch constants of U2: initUndistortRectifyMap's (fx, fy, u0, v0) = camera (0,0), (1,1), (0,2), (1,2); distortion k1 k2 p1 p2 k3
// (k4..k6 = s1..s4 = 0: a 5-element vector); the row term of the inverse, y = (i * ir[4] + ir[5]) * (1 / _w) with _w = ir[8] -- zero-skew
// cameras only (the host refuses others), for which _y and _w do not move along a row.
struct UndistortParams { double fx, fy, u0, v0, k1, k2, p1, p2, k3, ir4, ir5, winv; };

// U2: one output pixel per (capture, row, column), four columns per lane; the undistorted RGB8 capture, any width. xt: the column table
// (x = _x * (1 / _w) per column, host-computed: undistort_column_table). k1s / oks: per-capture k1 and "calibration succeeded" (nullptr: params.k1
// and every capture). A capture with ok = 0 is its RGB conversion, unmoved (the CLI's img stays as it was, cimbar.cpp:139-141).
constexpr int UD_ROWS = 4;
template <int FMT>
__global__ __launch_bounds__(256) void k_undistort(const uint8_t* __restrict__ img, int w, int h, const double* __restrict__ xt, UndistortParams P,
                                                   const double* __restrict__ k1s, const int* __restrict__ oks, uint8_t* __restrict__ out, int xcd_order)
{
	int bx, by;
	xcd_tile(xcd_order, bx, by);
	const int f = blockIdx.z, x0 = bx * 64 + (threadIdx.x & 15) * 4;
	if (x0 >= w) return;
	const uint8_t* src = img + (size_t)f * capture_bytes((size_t)w, (size_t)h, FMT);
	uint8_t* dst = out + (size_t)f * w * h * 3;
	const bool ok = oks ? oks[f] != 0 : true;
	const double k1 = k1s ? k1s[f] : P.k1;
	const int nx = w - x0 < 4 ? w - x0 : 4;
	double xs[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) xs[k] = xt[k < nx ? x0 + k : x0];
#pragma unroll 1
	for (int it = 0; it < UD_ROWS; ++it) {
		const int y = (by * UD_ROWS + it) * 16 + (threadIdx.x >> 4);
		if (y >= h) break;
		const double yy = ((double)y * P.ir4 + P.ir5) * P.winv;
		const double y2 = yy * yy;
		uint32_t px[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			if (!ok) { px[k] = k < nx ? px_clean(capture_px(src, w, h, FMT, x0 + k, y)) : 0u; continue; }   // (px_clean: the pixels are shifted into each other below)
			// initUndistortRectifyMap's per-pixel body (undistort.simd.hpp, the scalar tail), identity tilt, k4..k6 = s1..s4 = 0: the denominator
			// 1 + ((k6 r2 + k5) r2 + k4) r2 is exactly 1 and the s terms add zeros
			const double x = xs[k];
			const double x2 = x * x;
			const double r2 = x2 + y2, _2xy = 2 * x * yy;
			const double kr = 1 + ((P.k3 * r2 + P.k2) * r2 + k1) * r2;
			const double xd = x * kr + P.p1 * _2xy + P.p2 * (r2 + 2 * x2);
			const double yd = yy * kr + P.p1 * (r2 + 2 * y2) + P.p2 * _2xy;
			const float u = (float)(P.fx * xd + P.u0), v = (float)(P.fy * yd + P.v0);   // CV_32FC1 maps
			// remap: cvRound(map * INTER_TAB_SIZE) in float (out of int range or NaN: INT_MIN, as cvtss2si)
			const float U = u * 32.f, V = v * 32.f;
			const int X = (U >= -2147483648.f && U < 2147483648.f) ? (int)rintf(U) : INT_MIN;
			const int Y = (V >= -2147483648.f && V < 2147483648.f) ? (int)rintf(V) : INT_MIN;
			px[k] = remap_bilinear<FMT>(src, w, h, X, Y);
		}
		uint8_t* o = dst + ((size_t)y * w + x0) * 3;
		if (nx == 4 && (w & 3) == 0) {
			uint32_t* o4 = reinterpret_cast<uint32_t*>(o);      // (w % 4 == 0, x0 % 4 == 0: the 12 bytes start on a dword)
			o4[0] = px[0] | (px[1] << 24);
			o4[1] = (px[1] >> 8) | (px[2] << 16);
			o4[2] = (px[2] >> 16) | (px[3] << 8);
		} else {
			for (int k = 0; k < nx; ++k) { o[3 * k] = (uint8_t)px[k]; o[3 * k + 1] = (uint8_t)(px[k] >> 8); o[3 * k + 2] = (uint8_t)(px[k] >> 16); }
		}
	}
}

// explicit parameters (Undistort::set_distortion_params): every capture "succeeds" with the given k1
__global__ __launch_bounds__(64) void k_undistort_fill(int n, double k1, int* __restrict__ ok_out, double* __restrict__ k1_out)
{
	const int f = blockIdx.x * 64 + threadIdx.x;
	if (f >= n) return;
	ok_out[f] = 1;
	k1_out[f] = k1;
}
#pragma clang fp contract(fast)
