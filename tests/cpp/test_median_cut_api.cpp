// The median-cut quantizer's place in the C++ API (include/quant_amd/Quantizer.hpp), host side: no
// engine call is reached.  Driven by tests/test_median_cut_cpu.py.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "quant_amd/Compressor.hpp"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            failures++;                                                       \
        }                                                                     \
    } while (0)

int main() {
    // getQuantizer is the reference's: LBG only
    CHECK(getQuantizer(Quantizers::MEDIAN_CUT) == nullptr);
    CHECK(getQuantizer(Quantizers::LBG_MEDIAN_CUT) == nullptr);
    CHECK(getQuantizer(Quantizers::ABC) == nullptr);
    CHECK(getQuantizer(Quantizers::LBG) != nullptr);
    // the new factory
    CHECK(getMedianCutQuantizer() != nullptr);
    CHECK(getMedianCutQuantizer(5) != nullptr);
    CHECK(getMedianCutQuantizer(0, true) != nullptr);
    CHECK(getMedianCutQuantizer(3, false, true) != nullptr);
    bool threw = false;
    try {
        getMedianCutQuantizer(0, false, true);   // reseed needs refineIters > 0
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    // compress: CIE1931 has no median cut, ABC no implementation -- both before any engine call
    RGBImage img;
    img.xSize = img.ySize = 2;
    img.img.assign(4, RGB{1, 2, 3});
    for (Quantizers q : {Quantizers::MEDIAN_CUT, Quantizers::LBG_MEDIAN_CUT}) {
        std::string what;
        try {
            CompressedImage::compress(img, q, ColorSpaces::CIE1931, 2, 2, 1e-6, 1);
        } catch (const std::runtime_error &e) {
            what = e.what();
        }
        CHECK(what.find("median cut has no exact mode") != std::string::npos);
    }
    std::string what;
    try {
        CompressedImage::compress(img, Quantizers::ABC, ColorSpaces::SCALED, 2, 2, 1e-6, 1);
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    CHECK(what.find("quantizer not implemented") != std::string::npos);
    if (failures) return 1;
    std::puts("median cut api ok");
    return 0;
}
