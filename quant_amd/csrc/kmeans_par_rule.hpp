// kmeans_par_rule.hpp -- the arithmetic qvq_kmeans_par's rule adds to kmeanspp_rule.hpp (include/qvq.h;
// DESIGN.md 3.17): the round's key, a row's sampling test and the packed key of the update.  The
// kernels of k_kmeans_par.hip and the host helper qvq_host_kmeans_par_join run this text.  Integers only.
#pragma once
#include "kmeanspp_rule.hpp"

namespace qvq {

// The reduction draws from the stream seed + 2^32 (the sampling rounds use seed + 1 .. seed + 16,
// candidate 0 draw(seed, 0, N)).
__host__ __device__ inline uint64_t kmpar_reduce_seed(uint64_t seed) { return seed + (1ull << 32); }

// key_r = mix(seed + r), r = 1 .. rounds
__host__ __device__ inline uint64_t kmpar_round_key(uint64_t seed, uint32_t r) { return kmpp_mix(seed + r); }

__host__ __device__ inline uint64_t kmpar_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Row `row` joins round r's sample iff mulhi64(mix(key_r + row), phi) < ell * m: strict, so a row with
// m = 0 never joins.  ell <= 2^17 and m < 2^22: the right side is below 2^39.
__host__ __device__ inline bool kmpar_joins(uint64_t key, uint64_t row, uint64_t phi, uint32_t ell, uint32_t m) {
    return kmpar_mulhi(kmpp_mix(key + row), phi) < (uint64_t)ell * m;
}

// The update's packed key: the weight above the candidate's index within its chunk, so that one
// unsigned min carries both and the lowest index keeps a tie.  w < 2^22: the key is below 2^32.
constexpr uint32_t KMPAR_IDX_BITS = 10;
__host__ __device__ inline uint32_t kmpar_pack(uint32_t w, uint32_t idx) { return (w << KMPAR_IDX_BITS) | idx; }
__host__ __device__ inline uint32_t kmpar_key_weight(uint32_t key) { return key >> KMPAR_IDX_BITS; }
__host__ __device__ inline uint32_t kmpar_key_index(uint32_t key) { return key & ((1u << KMPAR_IDX_BITS) - 1); }

}  // namespace qvq
