// quant_amd C++ API -- the quantizer plugin interface (reference: include/Quantizer.hpp:8-20,
// src/Quantizer.cpp:119-155), with LBG running on the MI355X engine (include/qvq.h).
#pragma once
#include <cstddef>
#include <cstdint>
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
// Split-LBG with Lloyd iterations at every level on the device (qvq_lbg_lloyd, include/qvq.h: the
// textbook schedule, the rule is written there): after every split up to lloydIters iterations,
// stopped by quantize()'s eps; reseed: the iterations reseed their empty cells (QVQ_LLOYD_RESEED,
// and QVQ_REFINE_RESEED for the refinement).  With refineIters > 0 or fresh, qvq_refine then
// continues at the final K as getRefinedLBGQuantizer's does.  lloydIters == 0 is
// std::invalid_argument.  Byte images only: any other training set (CIE1931 values included) throws
// std::runtime_error with the engine's message.  The codebook is converted to bytes as the engine
// returns it: there is no reference value to match.
QuantizerPtr getLloydLBGQuantizer(size_t lloydIters, bool reseed, size_t refineIters = 0, bool fresh = false);
// Median cut on the device (qvq_median_cut, include/qvq.h: the rule is written there; the reference
// names MEDIAN_CUT and LBG_MEDIAN_CUT and implements neither, so getQuantizer keeps giving nullptr
// for them).  quantize(trainingSet, n, eps) cuts to 2^n boxes; with refineIters > 0 or fresh it then
// runs qvq_refine as a warm start from the median-cut codebook (eps the stop rule, the flags as
// given).  reseed needs refineIters > 0 (std::invalid_argument otherwise).  Byte images only: any
// other training set throws std::runtime_error with the engine's message.
QuantizerPtr getMedianCutQuantizer(size_t refineIters = 0, bool fresh = false, bool reseed = false);
// k-means++ seeding on the device (qvq_kmeanspp, include/qvq.h: the rule is written there) and Lloyd
// refinement from the seeds.  quantize(trainingSet, n, eps) seeds K = 2^n code vectors with `seed`,
// then runs qvq_refine with C_start = the seeds, up to refineIters iterations stopped by eps and the
// flags as given; with refineIters == 0 it passes QVQ_REFINE_FRESH, so the returned assignment is the
// nearest seed.  reseed needs refineIters > 0 (std::invalid_argument otherwise).  Byte images only:
// any other training set throws std::runtime_error with the engine's message.  getQuantizer and the
// Quantizers enum have no slot for it (3 is the reference's ABC); compress() records LBG.
QuantizerPtr getKMeansPPQuantizer(uint64_t seed, size_t refineIters = 0, bool fresh = false, bool reseed = false);
// The same with k-means|| seeding (qvq_kmeans_par, include/qvq.h, default options): a few passes over
// the rows in place of K - 1.  n <= 16.
QuantizerPtr getKMeansParQuantizer(uint64_t seed, size_t refineIters = 0, bool fresh = false, bool reseed = false);
// The same with greedy k-means++ seeding (qvq_kmeanspp_greedy, include/qvq.h): `trials` candidate rows
// a round, the one that lowers the potential most is kept.  trials in 0 .. 16, 0 the default count
// (std::invalid_argument otherwise).
QuantizerPtr getGreedyKMeansPPQuantizer(uint64_t seed, unsigned trials = 0, size_t refineIters = 0, bool fresh = false,
                                        bool reseed = false);
