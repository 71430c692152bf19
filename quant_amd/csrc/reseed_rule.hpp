// reseed_rule.hpp -- the empty-cell reseed rule of qvq_refine (QVQ_REFINE_RESEED, include/qvq.h;
// DESIGN.md 3.11), in one place: the per-row error and its quantisation, the far-row key and the
// donors' order.  The row pass and the select of k_reseed.hip and the host helpers
// (qvq_host_row_error, qvq_host_reseed_far_key, qvq_host_reseed_select) run this text.
//
// Built with -ffp-contract=off on both sides: every subtraction, product and sum below is rounded
// once to fp64, in the order written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qvq {

// The quantisation's shift s: q = floor(e 2^s).  SCALED: e <= 64 (values in [0, 1], dim <= 64),
// s = 24; NORMAL: e <= 64 * 255^2, s = 8.  Either way q < 2^31.
__host__ __device__ inline int reseed_shift(bool scaled) { return scaled ? 24 : 8; }

// One component's step of the per-row error: e + (x - c)^2.
__host__ __device__ inline double reseed_error_step(double e, double x, double c) {
    const double u = x - c;
    return e + u * u;
}

// floor(e 2^s) as an unsigned integer (the scaling by a power of two is exact; e >= 0).  The
// clamp is never reached by a row and a centroid of one colour space's value range.
__host__ __device__ inline uint32_t reseed_quantise(double e, int s) {
    const double v = e * (double)(1ull << s);
    return v >= 2147483647.0 ? 0x7FFFFFFFu : (uint32_t)v;
}

// The per-row quantised error of values x (lookups of the row's codes: x_of(d)) against the code
// vector c, components 0 .. dim - 1 in ascending order.
template <typename XOf>
__host__ __device__ inline uint32_t reseed_row_error(XOf x_of, const double *c, uint32_t dim, int s) {
    double e = 0.0;
    for (uint32_t d = 0; d < dim; d++) e = reseed_error_step(e, x_of(d), c[d]);
    return reseed_quantise(e, s);
}

// The far-row key: a u64 max over a cell's rows gives the largest q first, then the lowest row.
__host__ __device__ inline uint64_t reseed_far_key(uint32_t q, uint32_t row) {
    return ((uint64_t)q << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__host__ __device__ inline uint32_t reseed_far_row(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull); }

// A cell of n rows and summed error E gives a seed: it keeps a row, and has an error to shed.
__host__ __device__ inline bool reseed_is_donor(uint64_t n, uint64_t E) { return n >= 2 && E > 0; }

// Donor (Ea, ka) gives before donor (Eb, kb): the larger E first, on equal E the lower k.
__host__ __device__ inline bool reseed_before(uint64_t Ea, uint32_t ka, uint64_t Eb, uint32_t kb) {
    return Ea != Eb ? Ea > Eb : ka < kb;
}

}  // namespace qvq
