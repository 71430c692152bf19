// The k-means++ quantizer's place in the C++ API (include/quant_amd/Quantizer.hpp), host side: no
// engine call is reached.  Driven by tests/test_kmeanspp_cpu.py.
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
    // getQuantizer and the enum are the reference's: no slot for k-means++
    CHECK(getQuantizer(Quantizers::ABC) == nullptr);
    CHECK((int)Quantizers::ABC == 3);
    CHECK(getQuantizer(Quantizers::LBG) != nullptr);
    // the new factory: any seed, the defaults, every legal combination
    CHECK(getKMeansPPQuantizer(0) != nullptr);
    CHECK(getKMeansPPQuantizer(0xFFFFFFFFFFFFFFFFull) != nullptr);
    CHECK(getKMeansPPQuantizer(7, 5) != nullptr);
    CHECK(getKMeansPPQuantizer(7, 0, true) != nullptr);
    CHECK(getKMeansPPQuantizer(7, 3, false, true) != nullptr);
    CHECK(getKMeansPPQuantizer(7, 3, true, true) != nullptr);
    for (bool fresh : {false, true}) {
        bool threw = false;
        try {
            getKMeansPPQuantizer(7, 0, fresh, true);   // reseed needs refineIters > 0
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        CHECK(threw);
    }
    // quantize's own checks come before any engine call
    QuantizerPtr q = getKMeansPPQuantizer(1);
    std::string what;
    try {
        q->quantize({}, 2, 1e-6);
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    CHECK(what.find("empty training set") != std::string::npos);
    what.clear();
    try {
        q->quantize({Vector(3, 0.0)}, 21, 1e-6);
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    CHECK(what.find("bits must be <= 20") != std::string::npos);
    what.clear();
    try {
        q->quantize({Vector(3, 0.0), Vector(2, 0.0)}, 2, 1e-6);
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    CHECK(what.find("different sizes") != std::string::npos);
    if (failures) return 1;
    std::puts("kmeans++ api ok");
    return 0;
}
