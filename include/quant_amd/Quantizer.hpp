// quant_amd C++ API -- the quantizer plugin interface (reference: include/Quantizer.hpp:8-20,
// src/Quantizer.cpp:119-155), with LBG running on the MI355X engine (include/qvq.h).
#pragma once
#include <cstddef>
#include <memory>
#include <tuple>
#include <vector>

#include "VectorOperations.hpp"

enum class Quantizers { LBG, MEDIAN_CUT, LBG_MEDIAN_CUT, ABC };

class AbstractQuantizer {
public:
    // (codebook 2^n x D, assigned code vector per training vector, distortion)
    virtual std::tuple<std::vector<Vector>, std::vector<size_t>, VectorType> quantize(
        const std::vector<Vector> &trainingSet, size_t n, VectorType eps) = 0;
    virtual ~AbstractQuantizer() = default;
};

typedef std::unique_ptr<AbstractQuantizer> QuantizerPtr;

// LBG -> the engine's split-LBG on HIP device QVQ_DEVICE (default 0); the other
// enumerators have no implementation, as in the reference, and give nullptr.
QuantizerPtr getQuantizer(Quantizers);
// The LBG quantizer followed by Lloyd refinement at the final K on the device (qvq_refine,
// include/qvq.h): up to maxIters iterations, stopped when no index changes or when the
// distortion's relative change falls to quantize()'s eps; fresh: the returned indices are the
// nearest code vectors of the returned codebook (one more assignment); reseed: after each
// iteration's centroid step the empty cells take rows of the worst cells (QVQ_REFINE_RESEED; byte
// images only, needs maxIters > 0: std::invalid_argument otherwise).  (0, false) is getQuantizer(LBG).
QuantizerPtr getRefinedLBGQuantizer(size_t maxIters, bool fresh, bool reseed = false);
