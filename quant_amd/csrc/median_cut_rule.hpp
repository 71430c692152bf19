// median_cut_rule.hpp -- the median-cut rule of qvq_median_cut (include/qvq.h), in
// one place: a code byte's ordinal, a box's cut axis from its per-component ranges, and the cut
// value from the 256-bin histogram on that axis.  The kernels of k_mediancut.hip and the host
// helpers (qvq_host_median_cut_axis, qvq_host_median_cut_select) run this text.  Integers only:
// nothing here depends on an order of evaluation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qvq {

// u = (int8)b + 128: both byte colour spaces order their code bytes by it (make_terms).
__host__ __device__ inline uint32_t mc_ordinal(uint32_t byte) { return (byte & 255u) ^ 0x80u; }

// The cut axis of a box: the component with the largest hi - lo, on equal ranges the lowest.
// *range takes that range.  An empty box has lo > hi in every component: range 0, axis 0.
__host__ __device__ inline uint32_t mc_axis(const uint32_t *lo, const uint32_t *hi, uint32_t dim, uint32_t *range) {
    uint32_t axis = 0, best = 0;
    for (uint32_t d = 0; d < dim; d++) {
        const uint32_t r = hi[d] > lo[d] ? hi[d] - lo[d] : 0;
        if (r > best) best = r, axis = d;
    }
    *range = best;
    return axis;
}

// How far the split after bin v, with cum rows at or below it, is from halving n rows: |2 cum - n|.
__host__ __device__ inline uint64_t mc_balance(uint64_t cum, uint64_t n) {
    const uint64_t twice = 2 * cum;
    return twice > n ? twice - n : n - twice;
}
// A candidate cut as one key: the minimum over v of mc_cut_key(balance, v) is the best balance and,
// on ties, the lowest v (balance <= 2^33, v < 256).
__host__ __device__ inline uint64_t mc_cut_key(uint64_t balance, uint32_t v) { return (balance << 8) | v; }

// The cut of a box of n rows whose ordinals on the axis span [lo, hi], hi > lo, and count h[v]:
// the v in [lo, hi - 1] that minimises |2 cum(v) - n|, cum(v) = sum of h[w] over w <= v, on ties the
// lowest.  Rows with u > t go to the upper child: h[lo] > 0 and h[hi] > 0 leave both non-empty.
// (The device's cut takes the same minimum of mc_cut_key over the bins with a block-wide scan.)
__host__ __device__ inline uint32_t mc_select(const uint32_t *h, uint32_t lo, uint32_t hi, uint64_t n) {
    uint64_t cum = 0, best = ~0ull;
    for (uint32_t v = lo; v < hi; v++) {
        cum += h[v];
        const uint64_t key = mc_cut_key(mc_balance(cum, n), v);
        if (key < best) best = key;
    }
    return (uint32_t)(best & 255u);
}

// A row of label b in a box that was cut at (axis, t) under `half` boxes: u > t takes b + half.
__host__ __device__ inline uint32_t mc_relabel(uint32_t b, uint32_t u, uint32_t t, uint32_t half) {
    return u > t ? b + half : b;
}

}  // namespace qvq
