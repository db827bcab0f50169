// cvshim_undistort.hpp -- test-side additions to the OpenCV stand-in (oracle/cvshim) for the reference's lens undistortion
// (extractor/Undistort.h, SimpleCameraCalibration.h/.cpp): Mat_<double> / Mat1d with the comma initializer, initUndistortRectifyMap and remap.
// Force-included (g++ -include) into every translation unit of tools/make_golden_undistort.py's harness; never part of the product.
#pragma once

// [assumed-OpenCV] Real OpenCV's headers pull in libstdc++'s <stdlib.h> / <math.h> wrappers, whose `using std::abs` makes the DOUBLE overload
// of abs() visible at global scope. Scanner::find_edge (Scanner.cpp:226-262) calls abs() on doubles; with the bare shim it would bind to C's
// int abs() and truncate. These two includes give the reference's sources the overload set a real OpenCV build sees.
#include <stdlib.h>
#include <math.h>

#include <opencv2/opencv.hpp>

namespace cv {

template <>
class Mat_<double> : public Mat
{
public:
	Mat_() {}
	Mat_(int r, int c) : Mat(r, c, CV_64F) {}
};
typedef Mat_<double> Mat1d;

#ifndef CVSHIM_HAS_BORDER_CONSTANT
enum { BORDER_CONSTANT = 0 };
#endif

// [assumed-OpenCV] undistort.dispatch.cpp / undistort.simd.hpp initUndistortRectifyMap(A, dist, R = Mat(), newCameraMatrix = A, size, CV_32FC1):
// iR = (A * I).inv() (lapack.cpp closed form for 3x3), per row i: _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8], then per
// column the scalar body and _x += ir[0], _y += ir[3], _w += ir[6] -- the running sums serially (OpenCV's SIMD body restarts them every few
// columns; the float cast hides that almost always). dist: 4 or 5 doubles (k1 k2 p1 p2 [k3]); k4..k6, s1..s4 = 0, tilt = identity.
inline void initUndistortRectifyMap(const Mat& camera, const Mat& dist, const Mat&, const Mat& newcam, Size size, int, Mat& map1, Mat& map2)
{
	double A[9], Ar[9], ir[9];
	for (int i = 0; i < 9; ++i) { A[i] = camera.ptr<double>(i / 3)[i % 3]; Ar[i] = newcam.ptr<double>(i / 3)[i % 3]; }
	if (!shim_detail::invert3x3(Ar, ir)) for (int i = 0; i < 9; ++i) ir[i] = 0;
	const int nd = dist.rows * dist.cols;
	const double* d = dist.ptr<double>(0);
	const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = nd >= 5 ? d[4] : 0., k4 = 0, k5 = 0, k6 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
	const double u0 = A[2], v0 = A[5], fx = A[0], fy = A[4];
	map1.create(size.height, size.width, CV_32FC1);
	map2.create(size.height, size.width, CV_32FC1);
	for (int i = 0; i < size.height; ++i)
	{
		float* m1f = map1.ptr<float>(i);
		float* m2f = map2.ptr<float>(i);
		double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
		for (int j = 0; j < size.width; ++j, _x += ir[0], _y += ir[3], _w += ir[6])
		{
			double w = 1. / _w, x = _x * w, y = _y * w;
			double x2 = x * x, y2 = y * y;
			double r2 = x2 + y2, _2xy = 2 * x * y;
			double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
			double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
			double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
			// matTilt = identity: vecTilt = (xd, yd, 1), invProj = 1
			double vt0 = 1 * xd + 0 * yd + 0 * 1., vt1 = 0 * xd + 1 * yd + 0 * 1., vt2 = 0 * xd + 0 * yd + 1 * 1.;
			double invProj = vt2 ? 1. / vt2 : 1;
			double u = fx * invProj * vt0 + u0;
			double v = fy * invProj * vt1 + v0;
			m1f[j] = (float)u;
			m2f[j] = (float)v;
		}
	}
}

// [assumed-OpenCV] imgwarp.cpp remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) for CV_8UC3 and CV_32FC1 maps: X = cvRound(map * 32) in
// float (cvtss2si: out of range / NaN -> INT_MIN), then the same fixed-point bilinear warpPerspective above uses: weights (32-fx)(32-fy)*32 ..
// (sum 2^15), taps outside the source = 0, out = (sum + 2^14) >> 15. In place (dst == src) works as in OpenCV (the source is cloned first).
inline void remap(const Mat& src_, Mat& dst, const Mat& map1, const Mat& map2, int, int)
{
	Mat src = src_.clone();
	const int sw = src.cols, sh = src.rows, W = map1.cols, H = map1.rows;
	Mat out(H, W, CV_8UC3);
	auto rnd = [](float f) -> int { return (f >= -2147483648.f && f < 2147483648.f) ? (int)lrintf(f) : INT_MIN; };
	auto sat16 = [](int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); };
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x)
		{
			const int X = rnd(map1.ptr<float>(y)[x] * 32.f), Y = rnd(map2.ptr<float>(y)[x] * 32.f);
			const int sx = sat16(X >> 5), sy = sat16(Y >> 5), fx = X & 31, fy = Y & 31;
			const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
			for (int c = 0; c < 3; ++c)
			{
				auto px = [&](int yy, int xx) -> int { return (xx < 0 || xx >= sw || yy < 0 || yy >= sh) ? 0 : src.ptr<uchar>(yy)[xx * 3 + c]; };
				const int v = px(sy, sx) * w00 + px(sy, sx + 1) * w01 + px(sy + 1, sx) * w10 + px(sy + 1, sx + 1) * w11;
				out.ptr<uchar>(y)[x * 3 + c] = (uchar)((v + (1 << 14)) >> 15);
			}
		}
	dst = out;
}

}  // namespace cv
