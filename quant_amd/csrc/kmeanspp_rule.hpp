// kmeanspp_rule.hpp -- the arithmetic of qvq_kmeanspp's rule (include/qvq.h) in one
// place: the random draw and the weight of two rows.  The kernels of k_kmeanspp.hip and the host
// helpers (qvq_host_kmpp_draw, qvq_host_kmpp_weight) run this text.  Integers only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qvq {

// A word of four code bytes as four ordinals o = (uint8)(code ^ 0x80) (mc_ordinal, median_cut_rule.hpp).
__host__ __device__ inline uint32_t kmpp_ordinals(uint32_t word) { return word ^ 0x80808080u; }

// splitmix64's output function; every operation wraps.
__host__ __device__ inline uint64_t kmpp_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// floor(mix(seed + j) * T / 2^64): the high half of the 128-bit product, in [0, T) for T > 0.
__host__ __device__ inline uint64_t kmpp_draw(uint64_t seed, uint64_t j, uint64_t T) {
    const uint64_t r = kmpp_mix(seed + j);
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(r, T);
#else
    return (uint64_t)(((unsigned __int128)r * T) >> 64);
#endif
}

// sum of a[i] * b[i] over the four bytes of two words, added to acc
__host__ __device__ inline uint32_t kmpp_dot4(uint32_t a, uint32_t b, uint32_t acc) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int i = 0; i < 32; i += 8) acc += ((a >> i) & 255u) * ((b >> i) & 255u);
    return acc;
#endif
}

// sum of o^2 over nw words of ordinals (at most 64 * 255^2 < 2^22)
__host__ __device__ inline uint32_t kmpp_norm(const uint32_t *o, uint32_t nw) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < nw; i++) n = kmpp_dot4(o[i], o[i], n);
    return n;
}

// w(a, b) = sum of (a - b)^2 over nw words of ordinals, as n_a + n_b - 2 a.b: exact in u32, every
// term below 2^23.  Pad bytes are equal in a and b and cancel.
__host__ __device__ inline uint32_t kmpp_weight(const uint32_t *a, uint32_t n_a, const uint32_t *b, uint32_t n_b,
                                                uint32_t nw) {
    uint32_t dot = 0;
    for (uint32_t i = 0; i < nw; i++) dot = kmpp_dot4(a[i], b[i], dot);
    return n_a + n_b - 2 * dot;
}

}  // namespace qvq
