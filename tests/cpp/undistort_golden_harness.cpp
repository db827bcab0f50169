// undistort_golden_harness.cpp -- the reference's own Undistort<SimpleCameraCalibration> + Extractor on raw RGB8 captures, compiled by
// tools/make_golden_undistort.py (build machine only) against the reference's sources over oracle/cvshim + tests/cpp/cvshim_undistort.hpp.
//   harness <w> <h> <capture.rgb> <undistorted.rgb> <frame.rgb> [14 params]
// prints: ok k1(%a) camera[9](%a) extract_status
#include "extractor/Extractor.h"
#include "extractor/SimpleCameraCalibration.h"
// the shim's Mat has no release(); Undistort::reset_distortion_params (never called here) names it: assigning an empty Mat is the same thing
#define release() operator=(cv::Mat())
#include "extractor/Undistort.h"
#undef release

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
	if (argc != 6 && argc != 20) { std::fprintf(stderr, "usage\n"); return 2; }
	const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
	std::vector<unsigned char> buf((size_t)w * h * 3);
	FILE* f = std::fopen(argv[3], "rb");
	if (!f || std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 3;
	std::fclose(f);
	cv::Mat img = cv::Mat(h, w, CV_8UC3, buf.data()).clone();
	bool ok;
	DistortionParameters dp;
	Undistort<SimpleCameraCalibration> und;
	if (argc == 20) {
		cv::Mat1d cam(3, 3), dist(1, 5);
		for (int i = 0; i < 9; ++i) cam.ptr<double>(i / 3)[i % 3] = std::atof(argv[6 + i]);
		for (int i = 0; i < 5; ++i) dist.ptr<double>(0)[i] = std::atof(argv[15 + i]);
		dp = DistortionParameters(cam, dist);
		ok = und.set_distortion_params(w, h, dp);
		if (ok) ok = und.undistort(img, img);
	} else {
		dp = Undistort<SimpleCameraCalibration>::get_distortion_parameters(img);
		ok = und.undistort(img, img);   // (computes the parameters again: the same scan)
	}
	f = std::fopen(argv[4], "wb");
	for (int y = 0; y < img.rows; ++y) std::fwrite(img.ptr<unsigned char>(y), 1, (size_t)img.cols * 3, f);
	std::fclose(f);
	Extractor ext;
	cv::Mat frame;
	const int status = ext.extract(img, frame);
	f = std::fopen(argv[5], "wb");
	if (status) for (int y = 0; y < frame.rows; ++y) std::fwrite(frame.ptr<unsigned char>(y), 1, (size_t)frame.cols * 3, f);
	std::fclose(f);
	std::printf("%d %a", ok ? 1 : 0, dp ? dp.distortion.ptr<double>(0)[0] : 0.0);
	for (int i = 0; i < 9; ++i) std::printf(" %a", dp ? dp.camera.ptr<double>(i / 3)[i % 3] : 0.0);
	std::printf(" %d\n", status);
	return 0;
}
