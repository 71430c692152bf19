// The Lloyd-per-level LBG quantizer's place in the C++ API (include/quant_amd/Quantizer.hpp), host
// side: no engine call is reached.  Compiled and run by tests/test_lbg_lloyd_cpu.py.
#include <cstdio>
#include <stdexcept>

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
    CHECK(getLloydLBGQuantizer(3, false) != nullptr);
    CHECK(getLloydLBGQuantizer(1, true) != nullptr);              // reseed needs no refinement here
    CHECK(getLloydLBGQuantizer(3, true, 4) != nullptr);
    CHECK(getLloydLBGQuantizer(3, false, 0, true) != nullptr);
    for (bool reseed : {false, true}) {
        bool threw = false;
        try {
            getLloydLBGQuantizer(0, reseed, 4);   // lloydIters == 0: getRefinedLBGQuantizer is the factory for that
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        CHECK(threw);
    }
    // the other factories keep their rules
    bool threw = false;
    try {
        getRefinedLBGQuantizer(0, false, true);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    CHECK(getQuantizer(Quantizers::LBG) != nullptr && getQuantizer(Quantizers::MEDIAN_CUT) == nullptr);
    // more than 20 bits is refused before anything reaches the engine
    QuantizerPtr q = getLloydLBGQuantizer(2, false);
    std::vector<Vector> rows(4, Vector(3, 0.5));
    threw = false;
    try {
        q->quantize(rows, 21, 1e-6);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);
    if (failures) return 1;
    std::puts("lbg lloyd api ok");
    return 0;
}
