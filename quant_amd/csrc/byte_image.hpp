// byte_image.hpp -- the value -> byte code rule of the fp64 training-set front door
// (qvq_set_vectors*, qvq_host_classify; the device pass in k_ingest.hip), in one place.
//
// A value is a byte's image under a colour space when its bits equal the bits of that space's
// table entry Terms::v64[code] (make_terms, engine.cpp: the reference's value under -ffast-math,
// SCALED = (s + 128) * fl(1/255)).  The rule only *guesses* the code by arithmetic and then compares
// bits against the table, so neither the host's nor the device's multiply, division or contraction
// has a say in which values pass: -0.0, NaN, +-Inf, denormals and every neighbour of a table value
// fail the comparison.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace qvq {

__host__ __device__ inline uint64_t f64_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
}

// all exponent bits set: +-Inf and NaN
__host__ __device__ inline bool f64_finite(double v) { return (f64_bits(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

// The code of v under SCALED (scaled) or NORMAL (v64: that space's Terms::v64), or -1 when v is no
// byte's image there.
//   SCALED: the candidate is u = (int)rint(v * 255) clamped to 0..255, the code u ^ 0x80
//           (v64[b] = ((int8)b + 128) * fl(1/255): u = b ^ 0x80 orders the bytes by value);
//   NORMAL: v in [-128, 127] truncated to an integer s, the code (uint8_t)(int8_t)s.
__host__ __device__ inline int byte_image_code(double v, bool scaled, const double *v64) {
    int code;
    if (scaled) {
        const double r = rint(v * 255.0);
        const int u = r >= 255.0 ? 255 : r >= 0.0 ? (int)r : 0;   // NaN: 0
        code = u ^ 0x80;
    } else {
        if (!(v >= -128.0 && v <= 127.0)) return -1;
        code = (int)(uint8_t)(int8_t)(int)v;
    }
    return f64_bits(v) == f64_bits(v64[code]) ? code : -1;
}

}  // namespace qvq
