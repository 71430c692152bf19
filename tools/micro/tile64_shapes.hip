// tile64_shapes.hip -- where the tile-to-fp64 pass spends its time: one 4096 x 4096
// raster of seeded bytes in bw x bh blocks (arguments, default 2 2) through
//   A  the engine's shape (k_tile64.hip): a lane writes its slot's 24 bytes as 8-byte stores,
//   B  the same slots staged in LDS and written as dense 16-byte-per-lane stores (output compared with A's),
//   W  a plain 16-byte-per-lane streaming store of the same 403 MB: the write roof of the session.
// Device ms from HIP events, 10 timed launches each after 2 untimed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iquant_amd/csrc tools/micro/tile64_shapes.hip \
//       -o tools/micro/tile64_shapes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cie1931.hpp"

using namespace qvq;

constexpr int T = 256, CAP = 2048;   // T64_THREADS, T64_GRID_CAP

struct Step {
    uint32_t dy, dx, j, i;
    uint64_t img;
};
struct Shape {
    uint64_t slots, pixels;
    uint32_t ySize, bw, bh, wB, hB;
    Step step;
};

__host__ __device__ inline Step digits(uint64_t s, uint32_t bw, uint32_t bh, uint32_t wB, uint32_t hB) {
    Step d;
    d.dy = (uint32_t)(s % bh), s /= bh;
    d.dx = (uint32_t)(s % bw), s /= bw;
    d.j = (uint32_t)(s % hB), s /= hB;
    d.i = (uint32_t)(s % wB), s /= wB;
    d.img = s;
    return d;
}

__device__ inline void advance(Step &at, const Shape &g) {
    uint32_t c;
    at.dy += g.step.dy, c = at.dy >= g.bh, at.dy -= c ? g.bh : 0;
    at.dx += g.step.dx + c, c = at.dx >= g.bw, at.dx -= c ? g.bw : 0;
    at.j += g.step.j + c, c = at.j >= g.hB, at.j -= c ? g.hB : 0;
    at.i += g.step.i + c, c = at.i >= g.wB, at.i -= c ? g.wB : 0;
    at.img += g.step.img + c;
}

__device__ inline void slot_values(const uint8_t *rgb, const Step &at, const Shape &g, bool live, double v[3]) {
    const uint64_t px = ((uint64_t)at.i * g.bw + at.dx) * g.ySize + ((uint64_t)at.j * g.bh + at.dy);
    v[0] = v[1] = v[2] = 0.0;
    if (live && px < g.pixels) {
        const uint8_t *p = rgb + (at.img * g.pixels + px) * 3;
        cie1931_from_rgb((signed char)p[0], (signed char)p[1], (signed char)p[2], v);
    }
}

__global__ void __launch_bounds__(T) shape_a(const uint8_t *__restrict__ rgb, double *__restrict__ X, Shape g) {
    const uint64_t stride = (uint64_t)gridDim.x * T;
    uint64_t s = (uint64_t)blockIdx.x * T + threadIdx.x;
    Step at = digits(s, g.bw, g.bh, g.wB, g.hB);
    for (; s < g.slots; s += stride) {
        double v[3];
        slot_values(rgb, at, g, true, v);
        double *o = X + 3 * s;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        advance(at, g);
    }
}

typedef double f64x2 __attribute__((ext_vector_type(2)));

// the block's 256 slots are one dense run of 6144 bytes at X + 3 * base: 384 chunks of 16 bytes
__global__ void __launch_bounds__(T) shape_b(const uint8_t *__restrict__ rgb, double *__restrict__ X, Shape g) {
    __shared__ __attribute__((aligned(16))) double stage[3 * T];
    const uint64_t stride = (uint64_t)gridDim.x * T;
    uint64_t base = (uint64_t)blockIdx.x * T;   // uniform over the block: the barriers below are safe
    Step at = digits(base + threadIdx.x, g.bw, g.bh, g.wB, g.hB);
    for (; base < g.slots; base += stride) {
        double v[3];
        slot_values(rgb, at, g, base + threadIdx.x < g.slots, v);
        stage[3 * threadIdx.x] = v[0];
        stage[3 * threadIdx.x + 1] = v[1];
        stage[3 * threadIdx.x + 2] = v[2];
        __syncthreads();
        const uint64_t left = g.slots - base;
        const uint32_t nd = 3 * (uint32_t)(left < T ? left : T);   // doubles of this trip
        double *o = X + 3 * base;
        for (uint32_t c = threadIdx.x; 2 * c < nd; c += T) {
            if (2 * c + 1 < nd) *reinterpret_cast<f64x2 *>(o + 2 * c) = *reinterpret_cast<const f64x2 *>(stage + 2 * c);
            else o[2 * c] = stage[2 * c];
        }
        __syncthreads();
        advance(at, g);
    }
}

__global__ void __launch_bounds__(T) shape_w(f64x2 *__restrict__ X, uint64_t n16) {
    const uint64_t stride = (uint64_t)gridDim.x * T;
    for (uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x; i < n16; i += stride) X[i] = f64x2{1.0, (double)i};
}

#define CK(x)                                                 \
    do {                                                      \
        hipError_t e_ = (x);                                  \
        if (e_ != hipSuccess) {                               \
            printf("%s: %s\n", #x, hipGetErrorString(e_));    \
            return 1;                                         \
        }                                                     \
    } while (0)

int main(int argc, char **argv) {
    const uint32_t S = 4096, bw = argc > 1 ? atoi(argv[1]) : 2, bh = argc > 2 ? atoi(argv[2]) : 2;
    Shape g;
    g.ySize = S, g.bw = bw, g.bh = bh;
    g.wB = (S + bw - 1) / bw, g.hB = (S + bh - 1) / bh;
    g.slots = (uint64_t)g.wB * g.hB * bw * bh, g.pixels = (uint64_t)S * S;
    const uint64_t nd = g.slots * 3;
    std::vector<uint8_t> h(g.pixels * 3);
    uint64_t z = 1;
    for (uint8_t &b : h) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(z >> 56);
    }
    uint8_t *rgb;
    double *XA, *XB;
    CK(hipMalloc(&rgb, h.size()));
    CK(hipMalloc(&XA, nd * 8));
    CK(hipMalloc(&XB, nd * 8));
    CK(hipMemcpy(rgb, h.data(), h.size(), hipMemcpyHostToDevice));
    const int grid = (int)std::min<uint64_t>((g.slots + T - 1) / T, CAP);
    g.step = digits((uint64_t)grid * T, bw, bh, g.wB, g.hB);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const char *names[3] = {"A 24B/lane", "B staged 16B", "W plain 16B"};
    for (int v = 0; v < 3; v++) {
        std::vector<float> ms;
        for (int r = 0; r < 12; r++) {
            CK(hipEventRecord(e0, 0));
            if (v == 0) hipLaunchKernelGGL(shape_a, dim3(grid), dim3(T), 0, 0, rgb, XA, g);
            if (v == 1) hipLaunchKernelGGL(shape_b, dim3(grid), dim3(T), 0, 0, rgb, XB, g);
            if (v == 2) hipLaunchKernelGGL(shape_w, dim3(grid), dim3(T), 0, 0, (f64x2 *)XA, nd / 2);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("%s %ux%u: median %.4f ms min %.4f max %.4f  (%.0f GB/s written)\n", names[v], bw, bh, ms[ms.size() / 2],
               ms.front(), ms.back(), nd * 8 / (ms[ms.size() / 2] * 1e6));
        if (v == 1) {   // before W overwrites XA
            std::vector<double> a(nd), b(nd);
            CK(hipMemcpy(a.data(), XA, nd * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(b.data(), XB, nd * 8, hipMemcpyDeviceToHost));
            printf("A == B: %s\n", memcmp(a.data(), b.data(), nd * 8) == 0 ? "yes" : "NO");
        }
    }
    return 0;
}
