// The lens-undistortion adapter (libcimbar_amd/host/Undistort.h) driven the way the reference's decode loop drives Undistort<SimpleCameraCalibration>
// (cimbar.cpp:135-145), against the numpy restatement's outputs (tests/test_gpu_undistort_adapter.py writes them):
//   test_undistort_adapter <dir>   with <dir>/{a,b}.rgb (1920x1080 captures), want_a.rgb (a, calibrated), want_b_cached.rgb (b with a's parameters),
//                                  want_b.rgb (b, calibrated), want_full.rgb (b with params.bin), params.bin (14 doubles), blank.rgb
#include "../../libcimbar_amd/host/Undistort.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using cimbar_amd::image;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static std::vector<unsigned char> load(const std::string& p)
{
	std::vector<unsigned char> v;
	FILE* f = std::fopen(p.c_str(), "rb");
	if (!f) return v;
	std::fseek(f, 0, SEEK_END);
	v.resize((size_t)std::ftell(f));
	std::fseek(f, 0, SEEK_SET);
	if (std::fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
	std::fclose(f);
	return v;
}

static image load_image(const std::string& p, int w, int h)
{
	image img(w, h, 3);
	const std::vector<unsigned char> v = load(p);
	if (v.size() == (size_t)w * h * 3) std::memcpy(img.data, v.data(), v.size());
	return img;
}

static bool same(const image& a, const std::vector<unsigned char>& want)
{
	if (want.size() != (size_t)a.cols * a.rows * 3) return false;
	for (int y = 0; y < a.rows; ++y)
		if (std::memcmp(a.data + (size_t)y * a.step, want.data() + (size_t)y * a.cols * 3, (size_t)a.cols * 3)) return false;
	return true;
}

int main(int argc, char** argv)
{
	if (argc != 2) return 2;
	const std::string d = argv[1];
	const int w = 1920, h = 1080;
	image a = load_image(d + "/a.rgb", w, h), b = load_image(d + "/b.rgb", w, h), blank = load_image(d + "/blank.rgb", w, h);

	// first call calibrates on its image, in place (cimbar.cpp:139: und.undistort(img, img))
	cimbar_amd::Undistort<cimbar_amd::SimpleCameraCalibration> und;
	image img = a;
	CHECK(und.undistort(img, img));
	CHECK(same(img, load(d + "/want_a.rgb")));
	// the second image reuses the cached parameters
	image out;
	CHECK(und.undistort(b, out));
	CHECK(same(out, load(d + "/want_b_cached.rgb")));
	// reset: the next image is calibrated again
	und.reset_distortion_params();
	CHECK(und.undistort(b, out));
	CHECK(same(out, load(d + "/want_b.rgb")));
	// explicit parameters
	const std::vector<unsigned char> pb = load(d + "/params.bin");
	CHECK(pb.size() == 14 * sizeof(double));
	double p[14] = {};
	if (pb.size() == sizeof p) std::memcpy(p, pb.data(), sizeof p);
	cimbar_amd::Undistort<cimbar_amd::SimpleCameraCalibration> und2;
	CHECK(und2.set_distortion_params(w, h, cimbar_amd::DistortionParameters(p, p + 9)));
	CHECK(und2.undistort(b, out));
	CHECK(same(out, load(d + "/want_full.rgb")));
	CHECK(!und2.set_distortion_params(w, h, cimbar_amd::DistortionParameters()));
	// no anchors: no parameters, undistort fails and leaves `out` alone
	CHECK(!cimbar_amd::Undistort<cimbar_amd::SimpleCameraCalibration>::get_distortion_parameters(blank));
	cimbar_amd::Undistort<cimbar_amd::SimpleCameraCalibration> und3;
	image keep = a;
	CHECK(!und3.undistort(blank, keep));
	CHECK(same(keep, load(d + "/a.rgb")));
	// and the extractor takes the undistorted capture
	cimbar_amd::Extractor ext(cimbar_amd::default_undistort_decoder());
	image frame;
	CHECK(ext.extract(img, frame) != cimbar_amd::Extractor::FAILURE && frame.cols == 1024 && frame.rows == 1024);
	if (fails) return 1;
	std::printf("OK\n");
	return 0;
}
