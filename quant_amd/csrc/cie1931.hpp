// cie1931.hpp -- the CIE1931 colour map of one pixel, in one place: Cie1931Space::RGBtoColorSpace
// (quant_amd/cpp/ColorSpace.cpp, the reference's src/ColorSpace.cpp:30-33), the tile-to-fp64 kernel
// (k_tile64.hip) and qvq_host_cie1931 all call it, so the C++ layer and the device cannot drift apart.
//
// The values are what the reference's expression gives when it is evaluated as written: every
// product and every sum rounded on its own, left to right, and a true fp64 division by 0.17697 (not
// a multiplication by its reciprocal); nothing is rebuilt from a table.  quant_amd/csrc/Makefile
// compiles every translation unit that includes this header with -ffp-contract=off, so neither the
// host's nor the device's compiler may fuse a product into a sum (a baseline x86-64 build has no FMA
// to fuse into; the flag covers -march=native and the like).  r * 0 stays in the expression: it
// is -0.0 for a negative r, which the sum with g * 0.01 (never -0.0) turns into the same bits as the
// reference's; no output is ever -0.0.
//
// Plain C++ for g++ (libquant_amd, the host sanitizer builds) and __host__ __device__ under hipcc.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QVQ_CIE_HD __host__ __device__
#else
#define QVQ_CIE_HD
#endif

namespace qvq {

// out[0..2] = X, Y, Z of the pixel whose three raster bytes, read as signed chars, are r, g, b.
QVQ_CIE_HD inline void cie1931_from_rgb(signed char r8, signed char g8, signed char b8, double out[3]) {
    const double r = r8, g = g8, b = b8, n = 0.17697;
    out[0] = ((r * 0.490 + g * 0.310) + b * 0.200) / n;
    out[1] = ((r * 0.17697 + g * 0.81240) + b * 0.01063) / n;
    out[2] = ((r * 0 + g * 0.01) + b * 0.99) / n;
}

}  // namespace qvq
