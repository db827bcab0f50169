// cimbar_amd::Undistort -- C++ host adapter over the C ABI's lens undistortion (include/cimbar_hip.h, cimbar_hip_undistort_*), with the
// reference's class shapes so that its decode loop (`cimbar --undistort`, cimbar.cpp:135-145) keeps its code:
//
//     reference                                                              here
//     ---------------------------------------------------------------------  --------------------------------------------------------------
//     class DistortionParameters    src/lib/extractor/DistortionParameters.h  cimbar_amd::DistortionParameters (camera[9], distortion[5], bool)
//     class SimpleCameraCalibration src/lib/extractor/SimpleCameraCalibration.h:13-58   cimbar_amd::SimpleCameraCalibration (scan(img))
//     template <CAMERA_CALIBRATOR> class Undistort   src/lib/extractor/Undistort.h:7-62   cimbar_amd::Undistort<CAMERA_CALIBRATOR>
//         get_distortion_parameters(img), undistort(img, out), set_distortion_params(w, h, params), reset_distortion_params()
//
// The caching is the reference's: the first undistort() derives the parameters from its image and keeps them; later calls on the same object reuse
// them (and the map size, the first image's). undistort() returns false and leaves `out` alone when no parameters can be derived. Default-constructed
// objects run on a process-wide context (device 0, mode B); the constructors taking a cimbar_amd::Decoder use that one's. A later image whose size
// differs from the map's is refused (false, `out` untouched) -- the reference would remap it onto the first image's size.
//
// Header-only, include after Decoder.h's directory is on the path; link against libcimbar_hip.so. No OpenCV requirement: MAT as for Decoder.h
// (cv::Mat, cv::UMat, cimbar_amd::image), three channels, RGB order.
#pragma once

#include "Decoder.h"

namespace cimbar_amd {

// the context default-constructed calibrators and undistorters run on
inline Decoder& default_undistort_decoder()
{
	static Decoder dec;
	return dec;
}

class DistortionParameters
{
public:
	double camera[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // row-major 3x3
	double distortion[5] = {0, 0, 0, 0, 0};           // k1 k2 p1 p2 k3 (the reference's calibrator fills four: k3 = 0 is the same map)

	DistortionParameters() {}
	DistortionParameters(const double cam[9], const double dist[5]) : _set(true)
	{
		for (int i = 0; i < 9; ++i) camera[i] = cam[i];
		for (int i = 0; i < 5; ++i) distortion[i] = dist[i];
	}

	// DistortionParameters.h: `camera.cols > 0`
	operator bool() const { return _set; }

protected:
	bool _set = false;
};

// implements CAMERA_CALIBRATOR (SimpleCameraCalibration.h:13-28): SimpleCameraCalibration::scan on the device (cimbar_hip_undistort_calibrate_fmt)
class SimpleCameraCalibration
{
public:
	SimpleCameraCalibration() : _dec(&default_undistort_decoder()) {}
	explicit SimpleCameraCalibration(Decoder& decoder) : _dec(&decoder) {}

	template <typename MAT>
	DistortionParameters scan(const MAT& img)
	{
		if (!_dec->good()) return {};
		int ok = 0;
		double k1 = 0;
		int w = 0, h = 0;
		const int rc = detail::with_mat(img, [&](const auto& m) {
			if (m.cols <= 0 || m.rows <= 0) return -1;
			w = m.cols; h = m.rows;
			std::vector<unsigned char> packed;
			const unsigned char* src = Deskewer::dense(m, packed);
			return cimbar_hip_undistort_calibrate_fmt(_dec->context(), src, (unsigned)w, (unsigned)h, 3, 1, CIMBAR_HIP_MEM_HOST, &ok, &k1, nullptr);
		});
		if (rc != 0 || !ok) return {};
		return naive_radial_undistort(w, h, k1);
	}

	// SimpleCameraCalibration.h:50-58: [w/4, 0, w/2; 0, h/4, h/2; 0, 0, 1] in integer division, distortion (k1, 0, 0, 0)
	static DistortionParameters naive_radial_undistort(int width, int height, double distortion_factor)
	{
		const double cam[9] = {(double)(width / 4), 0, (double)(width / 2), 0, (double)(height / 4), (double)(height / 2), 0, 0, 1};
		const double dist[5] = {distortion_factor, 0, 0, 0, 0};
		return DistortionParameters(cam, dist);
	}

protected:
	Decoder* _dec;
};

template <typename CAMERA_CALIBRATOR>
class Undistort
{
public:
	Undistort() : _dec(&default_undistort_decoder()) {}
	explicit Undistort(Decoder& decoder) : _dec(&decoder) {}

	Undistort(int width, int height, const DistortionParameters& params) : Undistort()
	{
		set_distortion_params(width, height, params);
	}

	template <typename MAT>
	static DistortionParameters get_distortion_parameters(const MAT& img)
	{
		return CAMERA_CALIBRATOR().scan(img);
	}

	// Undistort.h:25-36: cv::remap(img, out, map1, map2, INTER_LINEAR, BORDER_CONSTANT) with the cached parameters' map (cimbar_hip_undistort_batch_fmt
	// with explicit parameters); img and out may be the same object
	template <typename MAT>
	bool undistort(const MAT& img, MAT& out)
	{
		if (!_params)
		{
			if (!set_distortion_params(img.cols, img.rows, get_distortion_parameters(img)))
				return false;
		}
		if (!_dec->good() || img.cols != _width || img.rows != _height) return false;
		double p[14];
		for (int i = 0; i < 9; ++i) p[i] = _params.camera[i];
		for (int i = 0; i < 5; ++i) p[9 + i] = _params.distortion[i];
		std::vector<unsigned char> res((size_t)_width * _height * 3);
		int type = 0;
		const int rc = detail::with_mat(img, [&](const auto& m) {
			type = m.type();
			std::vector<unsigned char> packed;
			const unsigned char* src = Deskewer::dense(m, packed);
			return cimbar_hip_undistort_batch_fmt(_dec->context(), src, (unsigned)_width, (unsigned)_height, 3, 1, CIMBAR_HIP_MEM_HOST, p, res.data(),
			                                      CIMBAR_HIP_MEM_HOST, nullptr, nullptr, nullptr);
		});
		if (rc != 0) return false;
		out.create(_height, _width, type);
		detail::with_mat_rw(out, [&](auto& m) {
			for (int y = 0; y < _height; ++y)
				for (size_t k = 0; k < (size_t)_width * 3; ++k)
					m.data[(size_t)y * m.step + k] = res[(size_t)y * _width * 3 + k];
		});
		return true;
	}

	// Undistort.h:38-46
	bool set_distortion_params(int width, int height, const DistortionParameters& params)
	{
		if (!params)
			return false;
		_params = params;
		_width = width;
		_height = height;
		return true;
	}

	// Undistort.h:48-53
	void reset_distortion_params()
	{
		_params = {};
		_width = _height = 0;
	}

protected:
	Decoder* _dec;
	DistortionParameters _params;
	int _width = 0, _height = 0;   // the map's size (initUndistortRectifyMap's `size`)
};

}  // namespace cimbar_amd
