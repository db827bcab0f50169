// oracle/_ref/libcimbar_ref.so, continued: the colour classifier of the REFERENCE (CimbDecoder::get_best_color, CimbDecoder.cpp:168-200) under
// an explicit colour-correction matrix, over many inputs per call -- what tests/test_colour_casts.py compares exhaustively with the oracle.
// TEST INFRASTRUCTURE ONLY, compiled against oracle/cvshim like ref_capi.cpp (see oracle/Makefile). Nothing here re-implements reference logic.
#include "cimb_translator/CimbDecoder.h"
#include "cimb_translator/Config.h"

#include <cstdint>
#include <utility>

namespace {

struct ColourDecoder : CimbDecoder
{
	ColourDecoder() : CimbDecoder(cimbar::Config::symbol_bits(), cimbar::Config::color_bits(), cimbar::Config::dark(), 0xFF) {}
	void reset_ccm() { internal_ccm() = color_correction(); }
};

}

extern "C" {

// the thread's CCM set to an explicit matrix (CimbDecoder::update_color_correction), or made inactive (active == 0)
void ref_set_ccm(const float* m9, int active)
{
	ColourDecoder d;
	if (!active) { d.reset_ccm(); return; }
	cv::Matx<float, 3, 3> m;
	for (int i = 0; i < 9; ++i) m.val[i] = m9[i];
	d.update_color_correction(std::move(m));
}

// get_best_color over n (r, g, b) float triples with the thread's current CCM, in the configured mode's palette -> out[n]
int ref_best_color_batch(const float* rgb3n, unsigned n, uint8_t* out)
{
	ColourDecoder d;
	const unsigned mode = cimbar::Config::color_mode();
	for (unsigned i = 0; i < n; ++i) out[i] = (uint8_t)d.get_best_color(rgb3n[3 * i], rgb3n[3 * i + 1], rgb3n[3 * i + 2], mode);
	return (int)n;
}

}  // extern "C"
