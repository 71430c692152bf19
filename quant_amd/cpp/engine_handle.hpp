// One engine context per host thread for the C++ API (include/qvq.h underneath).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "quant_amd/Quantizer.hpp"
#include "qvq.h"

namespace quant_amd {

class EngineHandle {
public:
    static qvq_ctx *get();   // creates the context on first use (device QVQ_DEVICE, default 0)
    static void check(qvq_status st, const char *what);   // throws std::runtime_error
};

// The refinement an engine LBG quantizer was made with (getRefinedLBGQuantizer; 0 / false for
// getQuantizer(LBG)); false when q is not the engine's LBG quantizer.  Lets compress() train such
// a quantizer straight from the raster (device tiling) instead of from host-built vectors.
struct RefineOptions {
    size_t maxIters = 0;
    bool fresh = false;
    bool reseed = false;
    bool medianCut = false;   // the codebook starts from qvq_median_cut, and the refinement is a warm start from it
    size_t lloydIters = 0;    // > 0: qvq_lbg_lloyd with that many iterations per level in place of qvq_lbg (reseed
                              // then holds for the levels too); the refinement, if any, continues from it
    bool kmeanspp = false;    // the codebook starts from qvq_kmeanspp's seeds (kmeansppSeed); the refinement starts from
    uint64_t kmeansppSeed = 0;   // them, and with maxIters == 0 it is the fresh assignment alone
    int kmeansppTrials = -1;  // with kmeanspp, >= 0: the seeds are qvq_kmeanspp_greedy's with that trial count (0: its default)
    bool kmeansPar = false;   // with kmeanspp: the seeds are qvq_kmeans_par's (getKMeansParQuantizer), default options
};
bool engine_lbg_options(const AbstractQuantizer &q, RefineOptions &out);
// The same for the engine's median-cut quantizer (getMedianCutQuantizer): out.medianCut is set.
bool engine_median_cut_options(const AbstractQuantizer &q, RefineOptions &out);

// The same for the engine's k-means++ quantizer (getKMeansPPQuantizer; getKMeansParQuantizer: kmeansPar too):
// out.kmeanspp and the seed are set.
bool engine_kmeanspp_options(const AbstractQuantizer &q, RefineOptions &out);

}  // namespace quant_amd
