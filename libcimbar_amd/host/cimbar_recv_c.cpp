// cimbar_recv_c.cpp -> libcimbar_recv_hip.so: the reference's receive-side C symbols for the decode step (include/cimbar_recv_hip.h), over the C ABI
// of libcimbar_hip.so. Plain C++ (g++), no HIP headers, no OpenCV. What each function replaces:
//     cimbard_get_bufsize            /root/reference/src/lib/cimbar_js/cimbar_recv_js.cpp:143-146
//     cimbard_scan_extract_decode    cimbar_recv_js.cpp:148-189 (get_rgb :94-120, Extractor::extract, Decoder::decode_fountain, escrow_buffer_writer)
//     cimbard_configure_decode       cimbar_recv_js.cpp:272-288
// and, not in the reference, cimbard_hip_scan_extract_decode_auto (include/cimbar_recv_hip_auto.h): web/recv.js's auto mode in one call
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/cimbar_hip.h"
#include "../../include/cimbar_recv_hip.h"
#include "../../include/cimbar_recv_hip_auto.h"

#ifdef CIMBARD_HOST_REST
// A build of the reference that keeps the rest of its cimbar_recv_js.cpp (sink, zstd: host code) beside this file: its own configure -- renamed
// at compile time -- still has to run, it resets the sink and updates the thread's cimbar::Config for the functions that stay.
extern "C" int CIMBARD_HOST_REST(int mode_val);
#endif

namespace {

std::atomic<int> g_mode{68};
std::atomic<int> g_device{-1};

int device_ordinal()
{
	int d = g_device.load();
	if (d < 0) {
		const char* v = std::getenv("CIMBAR_HIP_DEVICE");
		d = v ? std::atoi(v) : 0;
		g_device.store(d);
	}
	return d;
}

// one decoder per calling thread, like the reference's thread_local Config + colour-correction matrix
struct ThreadDecoder {
	cimbar_hip_ctx* ctx = nullptr;
	int mode = 0, device = -1;
	std::string report;
	~ThreadDecoder() { if (ctx) cimbar_hip_destroy(ctx); }
	int ensure(int want_mode, int want_device)
	{
		if (ctx && mode == want_mode && device == want_device) return 0;
		if (ctx) { cimbar_hip_destroy(ctx); ctx = nullptr; }
		const int rc = cimbar_hip_create(want_device, want_mode, &ctx);
		if (rc != 0 || !ctx) {
			report = "cimbar_hip_create failed (" + std::to_string(rc) + "): no gfx950 device for the decode path";
			ctx = nullptr;
			return rc ? rc : CIMBAR_HIP_EHIP;
		}
		mode = want_mode;
		device = want_device;
		return 0;
	}
};
thread_local ThreadDecoder t_dec;

// the auto mode's decoder: one auto-detection object per calling thread over the web receiver's candidates (recv.js:346,378)
constexpr int AUTO_MODES[4] = {66, 68, 67, 4};
struct ThreadAuto {
	cimbar_hip_auto* a = nullptr;
	int device = -1;
	~ThreadAuto() { if (a) cimbar_hip_auto_destroy(a); }
	int ensure(int want_device)
	{
		if (a && device == want_device) return 0;
		if (a) { cimbar_hip_auto_destroy(a); a = nullptr; }
		const int rc = cimbar_hip_auto_create(want_device, AUTO_MODES, 4, &a);
		if (rc != 0 || !a) {
			t_dec.report = "cimbar_hip_auto_create failed (" + std::to_string(rc) + "): no gfx950 device for the decode path";
			a = nullptr;
			return rc ? rc : CIMBAR_HIP_EHIP;
		}
		device = want_device;
		return 0;
	}
};
thread_local ThreadAuto t_auto;

}  // namespace

extern "C" {

int cimbard_hip_set_device(int device)
{
	if (device < 0) return -1;
	g_device.store(device);
	return 0;
}

int cimbard_configure_decode(int mode_val)
{
	if (mode_val <= 0) mode_val = 68;          // (cimbar_recv_js.cpp:274-276)
	g_mode.store(mode_val);                    // the thread's context follows at its next frame; the sink reset is the host build's business
#ifdef CIMBARD_HOST_REST
	return CIMBARD_HOST_REST(mode_val);
#else
	return 0;
#endif
}

int cimbard_get_bufsize(void)
{
	return cimbar_hip_mode_bufsize(g_mode.load());
}

unsigned cimbard_get_report(unsigned char* buff, unsigned maxlen)
{
	const std::string& r = t_dec.report;
	const unsigned len = r.size() < maxlen ? (unsigned)r.size() : maxlen;
	if (len && buff) std::memcpy(buff, r.data(), len);
	return len;
}

// `format` as the reference's get_rgb reads it (cimbar_recv_js.cpp:94-120): 4, 12 and 420 are its cases, every other value is RGB8. libcimbar_hip
// gives five more values a meaning of its own (CIMBAR_HIP_FMT_NV21 / YUYV / UYVY / BGR / BGRA); this interface is the reference's and keeps the
// reference's meaning, so they are RGB8 here as they always were. The native formats are reached through cimbar_hip_* only.
static int reference_format(int format)
{
	return (format == CIMBAR_HIP_FMT_RGBA || format == CIMBAR_HIP_FMT_NV12 || format == CIMBAR_HIP_FMT_I420) ? format : CIMBAR_HIP_FMT_RGB;
}

int cimbard_scan_extract_decode(const unsigned char* imgdata, unsigned imgw, unsigned imgh, int format, unsigned char* bufspace, unsigned bufsize)
{
	format = reference_format(format);
	if (imgw == 0 || imgh == 0) return -1;
	const int mode = g_mode.load();
	const int frame_bytes = cimbar_hip_mode_bufsize(mode);
	if (bufsize < (unsigned)frame_bytes) return -2;          // (cimbar_recv_js.cpp:158-159)
	if (!imgdata || !bufspace) { t_dec.report = "null buffer"; return -4; }
	if (t_dec.ensure(mode, device_ordinal()) != 0) return -4;
	int32_t geo[CIMBAR_HIP_GEOMETRY_WORDS];
	if (cimbar_hip_geometry(t_dec.ctx, geo) != CIMBAR_HIP_GEOMETRY_WORDS) { t_dec.report = "geometry"; return -4; }
	const unsigned per = (unsigned)geo[4], cs = (unsigned)geo[5];
	uint8_t chunks[CIMBAR_HIP_MAX_FRAME_BYTES];
	uint32_t mask = 0;
	int status = 0;
	// The capture crosses to the device as the camera delivered it (`format` is passed through: the conversion get_rgb does on the host happens inside
	// the kernels that read the capture), extract and decode follow without leaving the device. Upstream always sharpens on this path (:166) and
	// uses the header-derived colour correction (Decoder::decode_fountain's default 2).
	const int64_t rc = cimbar_hip_scan_extract_decode_batch_fmt(t_dec.ctx, imgdata, imgw, imgh, format, 1, CIMBAR_HIP_MEM_HOST, /*preprocess*/ 1,
	                                                            /*color_correction*/ 2, chunks, &mask, &status, CIMBAR_HIP_MEM_HOST, nullptr);
	if (rc < 0) {
		t_dec.report = std::string("cimbar_hip_scan_extract_decode_batch_fmt failed (") + std::to_string((long long)rc) + "): " + cimbar_hip_last_error(t_dec.ctx);
		return -4;
	}
	if (status <= 0) { t_dec.report = "no frame found"; return -3; }          // Extractor::FAILURE (:170-171)
	unsigned used = 0;                                                        // escrow_buffer_writer: the delivered chunks, packed front to back
	for (unsigned j = 0; j < per; ++j)
		if (mask & (1u << j)) std::memcpy(bufspace + (size_t)cs * used++, chunks + (size_t)cs * j, cs);
	t_dec.report = "decoded " + std::to_string(used * cs) + " bytes" + (status == 2 ? " (needs sharpen)" : "");
	return (int)(used * cs);
}

int cimbard_hip_scan_extract_decode_auto(const unsigned char* imgdata, unsigned imgw, unsigned imgh, int format, unsigned char* bufspace,
                                         unsigned bufsize, int* mode_out)
{
	if (mode_out) *mode_out = 0;
	format = reference_format(format);
	if (imgw == 0 || imgh == 0) return -1;
	if (bufsize < (unsigned)cimbar_hip_mode_bufsize(68)) return -2;   // 7500: the largest cimbard_get_bufsize of 66 68 67 4
	if (!imgdata || !bufspace) { t_dec.report = "null buffer"; return -4; }
	if (t_auto.ensure(device_ordinal()) != 0) return -4;
	uint8_t slot[CIMBAR_HIP_MAX_FRAME_BYTES];
	uint32_t mask = 0;
	int mode = 0, status = 0;
	const int64_t rc = cimbar_hip_auto_scan_extract_decode_batch_fmt(t_auto.a, nullptr, 0, imgdata, imgw, imgh, format, 1, CIMBAR_HIP_MEM_HOST,
	                                                                 /*preprocess*/ 1, /*color_correction*/ 2, slot, &mask, &mode, &status,
	                                                                 CIMBAR_HIP_MEM_HOST, nullptr);
	if (rc < 0) {
		t_dec.report = std::string("cimbar_hip_auto_scan_extract_decode_batch_fmt failed (") + std::to_string((long long)rc) + "): " +
		               cimbar_hip_auto_last_error(t_auto.a);
		return -4;
	}
	if (status <= 0) { t_dec.report = "no frame found"; return -3; }
	if (mode_out) *mode_out = mode;
	if (mode == 0) { t_dec.report = "no mode delivered a chunk"; return 0; }
	const int per = mode == 66 ? 6 : (mode == 4 || mode == 8 ? 10 : 12), cs = cimbar_hip_mode_bufsize(mode) / per;
	unsigned used = 0;
	for (int j = 0; j < per; ++j)
		if (mask & (1u << j)) std::memcpy(bufspace + (size_t)cs * used++, slot + (size_t)cs * j, cs);
	t_dec.report = "mode " + std::to_string(mode) + ": decoded " + std::to_string(used * cs) + " bytes";
	return (int)(used * cs);
}

}  // extern "C"
