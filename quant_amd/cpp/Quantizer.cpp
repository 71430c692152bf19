// getQuantizer / the LBG quantizer on the engine; see include/quant_amd/Quantizer.hpp.
#include "quant_amd/Quantizer.hpp"

#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>

#include "engine_handle.hpp"

namespace quant_amd {

namespace {
struct CtxDeleter {
    void operator()(qvq_ctx *c) const { qvq_destroy(c); }
};
thread_local std::unique_ptr<qvq_ctx, CtxDeleter> t_ctx;
}  // namespace

qvq_ctx *EngineHandle::get() {
    if (!t_ctx) {
        const char *dev = std::getenv("QVQ_DEVICE");
        qvq_ctx *c = nullptr;
        const qvq_status st = qvq_create(dev ? std::atoi(dev) : 0, &c);
        if (st != QVQ_OK) throw std::runtime_error(std::string("qvq_create: ") + qvq_last_error(nullptr));
        t_ctx.reset(c);
    }
    return t_ctx.get();
}

void EngineHandle::check(qvq_status st, const char *what) {
    if (st == QVQ_OK) return;
    const char *msg = qvq_last_error(t_ctx.get());
    throw std::runtime_error(std::string(what) + " failed (status " + std::to_string((int)st) + "): " +
                             (msg ? msg : ""));
}

}  // namespace quant_amd

namespace {

// LBGQuantizer::quantize (src/Quantizer.cpp:119-144) on the engine.  The training set is
// copied into one flat fp64 array.  Byte images of the NORMAL or SCALED colour space take the
// byte engine; any other finite data (CIE1931 values, arbitrary doubles) the engine's exact
// mode, the reference's arithmetic; non-finite values: std::runtime_error.
// With refinement (getRefinedLBGQuantizer): qvq_refine continues at K = 2^n from the split levels'
// result, up to maxIters Lloyd iterations stopped by eps, and with fresh returns the indices of the
// returned codebook.  With Lloyd iterations per level (getLloydLBGQuantizer): qvq_lbg_lloyd in place
// of qvq_lbg.
class HipLBGQuantizer : public AbstractQuantizer {
    size_t maxIters_ = 0;
    bool fresh_ = false, reseed_ = false;
    size_t lloydIters_ = 0;

public:
    HipLBGQuantizer() = default;
    HipLBGQuantizer(size_t maxIters, bool fresh, bool reseed, size_t lloydIters = 0)
        : maxIters_(maxIters), fresh_(fresh), reseed_(reseed), lloydIters_(lloydIters) {}
    quant_amd::RefineOptions options() const { return {maxIters_, fresh_, reseed_, false, lloydIters_}; }
    std::tuple<std::vector<Vector>, std::vector<size_t>, VectorType> quantize(const std::vector<Vector> &trainingSet,
                                                                              size_t n, VectorType eps) override {
        using quant_amd::EngineHandle;
        if (trainingSet.empty()) throw std::runtime_error("LBG quantize: empty training set");
        if (lloydIters_ > 0 && n > 20) throw std::runtime_error("LBG quantize: bits must be <= 20");
        const size_t N = trainingSet.size(), D = trainingSet[0].size();
        std::vector<double> flat(N * D);
        for (size_t i = 0; i < N; i++) {
            if (trainingSet[i].size() != D) throw std::runtime_error("LBG quantize: vectors of different sizes");
            std::copy(trainingSet[i].begin(), trainingSet[i].end(), flat.begin() + i * D);
        }
        qvq_ctx *ctx = EngineHandle::get();
        EngineHandle::check(qvq_set_vectors(ctx, flat.data(), N, (uint32_t)D), "qvq_set_vectors");
        const size_t K = (size_t)1 << n;
        std::vector<double> C(K * D);
        std::vector<uint32_t> A(N);
        double distortion = 0;
        if (lloydIters_ > 0xFFFFFFFFull) throw std::runtime_error("LBG quantize: too many Lloyd iterations per level");
        if (lloydIters_ > 0)
            EngineHandle::check(qvq_lbg_lloyd(ctx, (uint32_t)n, (uint32_t)lloydIters_, eps,
                                              reseed_ ? QVQ_LLOYD_RESEED : 0u, C.data(), A.data(), &distortion, nullptr),
                                "qvq_lbg_lloyd");
        else
            EngineHandle::check(qvq_lbg(ctx, (uint32_t)n, eps, C.data(), A.data(), &distortion), "qvq_lbg");
        if (maxIters_ > 0 || fresh_) {
            if (maxIters_ > 0xFFFFFFFFull) throw std::runtime_error("LBG quantize: too many refinement iterations");
            EngineHandle::check(qvq_refine(ctx, (uint32_t)K, nullptr, (uint32_t)maxIters_, eps,
                                           (fresh_ ? QVQ_REFINE_FRESH : 0u) | (reseed_ ? QVQ_REFINE_RESEED : 0u),
                                           C.data(), A.data(), &distortion, nullptr, nullptr, nullptr),
                                "qvq_refine");
        }
        std::vector<Vector> codebook(K, Vector(D));
        for (size_t k = 0; k < K; k++) std::copy(C.begin() + k * D, C.begin() + (k + 1) * D, codebook[k].begin());
        return std::make_tuple(std::move(codebook), std::vector<size_t>(A.begin(), A.end()), distortion);
    }
};

// Median cut on the engine (qvq_median_cut), then optionally qvq_refine warm-started from its codebook.
class HipMedianCutQuantizer : public AbstractQuantizer {
    size_t maxIters_ = 0;
    bool fresh_ = false, reseed_ = false;

public:
    HipMedianCutQuantizer(size_t maxIters, bool fresh, bool reseed) : maxIters_(maxIters), fresh_(fresh), reseed_(reseed) {}
    quant_amd::RefineOptions options() const { return {maxIters_, fresh_, reseed_, true}; }
    std::tuple<std::vector<Vector>, std::vector<size_t>, VectorType> quantize(const std::vector<Vector> &trainingSet,
                                                                              size_t n, VectorType eps) override {
        using quant_amd::EngineHandle;
        if (trainingSet.empty()) throw std::runtime_error("median cut quantize: empty training set");
        if (n > 20) throw std::runtime_error("median cut quantize: bits must be <= 20");
        const size_t N = trainingSet.size(), D = trainingSet[0].size();
        std::vector<double> flat(N * D);
        for (size_t i = 0; i < N; i++) {
            if (trainingSet[i].size() != D) throw std::runtime_error("median cut quantize: vectors of different sizes");
            std::copy(trainingSet[i].begin(), trainingSet[i].end(), flat.begin() + i * D);
        }
        qvq_ctx *ctx = EngineHandle::get();
        EngineHandle::check(qvq_set_vectors(ctx, flat.data(), N, (uint32_t)D), "qvq_set_vectors");
        const size_t K = (size_t)1 << n;
        std::vector<double> C(K * D);
        std::vector<uint32_t> A(N);
        double distortion = 0;
        EngineHandle::check(qvq_median_cut(ctx, (uint32_t)n, C.data(), A.data(), &distortion, nullptr), "qvq_median_cut");
        if (maxIters_ > 0 || fresh_) {
            if (maxIters_ > 0xFFFFFFFFull) throw std::runtime_error("median cut quantize: too many refinement iterations");
            const std::vector<double> start = C;
            EngineHandle::check(qvq_refine(ctx, (uint32_t)K, start.data(), (uint32_t)maxIters_, eps,
                                           (fresh_ ? QVQ_REFINE_FRESH : 0u) | (reseed_ ? QVQ_REFINE_RESEED : 0u),
                                           C.data(), A.data(), &distortion, nullptr, nullptr, nullptr),
                                "qvq_refine");
        }
        std::vector<Vector> codebook(K, Vector(D));
        for (size_t k = 0; k < K; k++) std::copy(C.begin() + k * D, C.begin() + (k + 1) * D, codebook[k].begin());
        return std::make_tuple(std::move(codebook), std::vector<size_t>(A.begin(), A.end()), distortion);
    }
};

// k-means++ seeding on the engine (qvq_kmeanspp; par: k-means||, qvq_kmeans_par with its default
// options; trials >= 0: greedy k-means++, qvq_kmeanspp_greedy), then qvq_refine from the seeds.  With no iterations the refinement is the fresh assignment
// alone: the nearest seed of every row.
class HipKMeansPPQuantizer : public AbstractQuantizer {
    uint64_t seed_ = 0;
    size_t maxIters_ = 0;
    bool fresh_ = false, reseed_ = false, par_ = false;
    int trials_ = -1;

public:
    HipKMeansPPQuantizer(uint64_t seed, size_t maxIters, bool fresh, bool reseed, bool par = false, int trials = -1)
        : seed_(seed), maxIters_(maxIters), fresh_(fresh), reseed_(reseed), par_(par), trials_(trials) {}
    quant_amd::RefineOptions options() const {
        quant_amd::RefineOptions o;
        o.maxIters = maxIters_, o.fresh = fresh_, o.reseed = reseed_, o.kmeanspp = true, o.kmeansppSeed = seed_, o.kmeansPar = par_;
        o.kmeansppTrials = trials_;
        return o;
    }
    std::tuple<std::vector<Vector>, std::vector<size_t>, VectorType> quantize(const std::vector<Vector> &trainingSet,
                                                                              size_t n, VectorType eps) override {
        using quant_amd::EngineHandle;
        if (trainingSet.empty()) throw std::runtime_error("k-means++ quantize: empty training set");
        if (n > 20) throw std::runtime_error("k-means++ quantize: bits must be <= 20");
        if (par_ && n > 16) throw std::runtime_error("k-means|| quantize: bits must be <= 16");
        if (maxIters_ > 0xFFFFFFFFull) throw std::runtime_error("k-means++ quantize: too many refinement iterations");
        const size_t N = trainingSet.size(), D = trainingSet[0].size();
        std::vector<double> flat(N * D);
        for (size_t i = 0; i < N; i++) {
            if (trainingSet[i].size() != D) throw std::runtime_error("k-means++ quantize: vectors of different sizes");
            std::copy(trainingSet[i].begin(), trainingSet[i].end(), flat.begin() + i * D);
        }
        qvq_ctx *ctx = EngineHandle::get();
        EngineHandle::check(qvq_set_vectors(ctx, flat.data(), N, (uint32_t)D), "qvq_set_vectors");
        const size_t K = (size_t)1 << n;
        std::vector<double> start(K * D), C(K * D);
        std::vector<uint32_t> A(N);
        double distortion = 0;
        if (par_)
            EngineHandle::check(qvq_kmeans_par(ctx, (uint32_t)K, seed_, nullptr, start.data(), nullptr, nullptr, nullptr, nullptr),
                                "qvq_kmeans_par");
        else if (trials_ >= 0)
            EngineHandle::check(qvq_kmeanspp_greedy(ctx, (uint32_t)K, seed_, (uint32_t)trials_, start.data(), nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, nullptr),
                                "qvq_kmeanspp_greedy");
        else
            EngineHandle::check(qvq_kmeanspp(ctx, (uint32_t)K, seed_, start.data(), nullptr, nullptr, nullptr), "qvq_kmeanspp");
        const bool fresh = fresh_ || maxIters_ == 0;
        EngineHandle::check(qvq_refine(ctx, (uint32_t)K, start.data(), (uint32_t)maxIters_, eps,
                                       (fresh ? QVQ_REFINE_FRESH : 0u) | (reseed_ ? QVQ_REFINE_RESEED : 0u), C.data(),
                                       A.data(), &distortion, nullptr, nullptr, nullptr),
                            "qvq_refine");
        std::vector<Vector> codebook(K, Vector(D));
        for (size_t k = 0; k < K; k++) std::copy(C.begin() + k * D, C.begin() + (k + 1) * D, codebook[k].begin());
        return std::make_tuple(std::move(codebook), std::vector<size_t>(A.begin(), A.end()), distortion);
    }
};

}  // namespace

bool quant_amd::engine_kmeanspp_options(const AbstractQuantizer &q, RefineOptions &out) {
    const HipKMeansPPQuantizer *h = dynamic_cast<const HipKMeansPPQuantizer *>(&q);
    if (h) out = h->options();
    return h != nullptr;
}

bool quant_amd::engine_median_cut_options(const AbstractQuantizer &q, RefineOptions &out) {
    const HipMedianCutQuantizer *h = dynamic_cast<const HipMedianCutQuantizer *>(&q);
    if (h) out = h->options();
    return h != nullptr;
}

bool quant_amd::engine_lbg_options(const AbstractQuantizer &q, RefineOptions &out) {
    const HipLBGQuantizer *h = dynamic_cast<const HipLBGQuantizer *>(&q);
    if (h) out = h->options();
    return h != nullptr;
}

QuantizerPtr getQuantizer(Quantizers q) {
    if (q == Quantizers::LBG) return QuantizerPtr(new HipLBGQuantizer());
    return nullptr;
}

QuantizerPtr getRefinedLBGQuantizer(size_t maxIters, bool fresh, bool reseed) {
    if (reseed && maxIters == 0) throw std::invalid_argument("getRefinedLBGQuantizer: reseed needs maxIters > 0");
    return QuantizerPtr(new HipLBGQuantizer(maxIters, fresh, reseed));
}

QuantizerPtr getLloydLBGQuantizer(size_t lloydIters, bool reseed, size_t refineIters, bool fresh) {
    if (lloydIters == 0) throw std::invalid_argument("getLloydLBGQuantizer: lloydIters must be > 0");
    return QuantizerPtr(new HipLBGQuantizer(refineIters, fresh, reseed, lloydIters));
}

QuantizerPtr getMedianCutQuantizer(size_t refineIters, bool fresh, bool reseed) {
    if (reseed && refineIters == 0) throw std::invalid_argument("getMedianCutQuantizer: reseed needs refineIters > 0");
    return QuantizerPtr(new HipMedianCutQuantizer(refineIters, fresh, reseed));
}

QuantizerPtr getKMeansPPQuantizer(uint64_t seed, size_t refineIters, bool fresh, bool reseed) {
    if (reseed && refineIters == 0) throw std::invalid_argument("getKMeansPPQuantizer: reseed needs refineIters > 0");
    return QuantizerPtr(new HipKMeansPPQuantizer(seed, refineIters, fresh, reseed));
}

QuantizerPtr getGreedyKMeansPPQuantizer(uint64_t seed, unsigned trials, size_t refineIters, bool fresh, bool reseed) {
    if (trials > 16) throw std::invalid_argument("getGreedyKMeansPPQuantizer: trials must be in 0 .. 16");
    if (reseed && refineIters == 0) throw std::invalid_argument("getGreedyKMeansPPQuantizer: reseed needs refineIters > 0");
    return QuantizerPtr(new HipKMeansPPQuantizer(seed, refineIters, fresh, reseed, false, (int)trials));
}

QuantizerPtr getKMeansParQuantizer(uint64_t seed, size_t refineIters, bool fresh, bool reseed) {
    if (reseed && refineIters == 0) throw std::invalid_argument("getKMeansParQuantizer: reseed needs refineIters > 0");
    return QuantizerPtr(new HipKMeansPPQuantizer(seed, refineIters, fresh, reseed, true));
}
