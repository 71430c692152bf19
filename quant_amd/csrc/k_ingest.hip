// k_ingest.hip -- the fp64 training-set front door on the device (qvq_set_vectors*):
// one streaming kernel over row-major X [n][dim] in two forms,
//   classify: the three set-wide verdicts (every value a SCALED image, every value a NORMAL image,
//             every value finite), nothing else written;
//   pack:     the byte codes [n][Dp] under the colour space the verdicts chose.
// Both apply byte_image_code (byte_image.hpp) against the 256-entry tables in LDS; no value is ever
// recomputed from a byte on the device.
//
// One lane produces one 4-byte code word: components 4q .. 4q + 3 of one row, read as two 16-byte
// loads (the rows are only 8-byte aligned: the loads are typed so) or, in a row's last partial word,
// one by one; components past dim count as 0.0, whose code under either space is the pad code, so a
// row's pad bytes come out of the same rule.  Grid-stride over the n * Dp / 4 words under
// ING_GRID_CAP blocks; the word's (row, q) advances without a division.  All offsets are 64-bit.
#include "byte_image.hpp"
#include "common.hpp"

namespace qvq {

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef f64x2 f64x2_a8 __attribute__((aligned(8)));

template <bool PACK>
__global__ void __launch_bounds__(ING_THREADS)
ingest_kernel(const double *__restrict__ X, uint64_t n, uint32_t dim, uint32_t wpr, const double *__restrict__ tab,
              uint32_t cs, uint32_t *__restrict__ words, unsigned *__restrict__ verdict) {
    // classify: [0, 256) NORMAL, [256, 512) SCALED; pack: the chosen space's table only
    __shared__ double lut[PACK ? 256 : 512];
    if constexpr (PACK) {
        lut[threadIdx.x] = tab[256 * cs + threadIdx.x];
    } else {
        lut[threadIdx.x] = tab[threadIdx.x];
        lut[256 + threadIdx.x] = tab[256 + threadIdx.x];
    }
    __syncthreads();
    const bool scaled = cs == 1;   // QVQ_CS_SCALED
    const uint64_t total = n * wpr;
    const uint64_t stride = (uint64_t)gridDim.x * ING_THREADS;
    uint64_t w = (uint64_t)blockIdx.x * ING_THREADS + threadIdx.x;
    uint64_t row = w / wpr;
    uint32_t q = (uint32_t)(w % wpr);
    const uint64_t srow = stride / wpr;
    const uint32_t sq = (uint32_t)(stride % wpr);
    bool all_sc = true, all_nm = true, all_fin = true;
    for (; w < total; w += stride) {
        const uint32_t d0 = 4 * q;
        const double *p = X + row * dim + d0;
        double v[4];
        if (d0 + 4 <= dim) {
            const f64x2 a = *reinterpret_cast<const f64x2_a8 *>(p);
            const f64x2 b = *reinterpret_cast<const f64x2_a8 *>(p + 2);
            v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = d0 + j < dim ? p[j] : 0.0;
        }
        if constexpr (PACK) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) word |= ((uint32_t)byte_image_code(v[j], scaled, lut) & 0xFFu) << (8 * j);
            words[w] = word;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                all_sc &= byte_image_code(v[j], true, lut + 256) >= 0;
                all_nm &= byte_image_code(v[j], false, lut) >= 0;
                all_fin &= f64_finite(v[j]);
            }
        }
        row += srow;
        q += sq;
        if (q >= wpr) {
            q -= wpr;
            row++;
        }
    }
    if constexpr (!PACK) {
        // wave reduction, then one atomic per workgroup (none when the workgroup objects to nothing)
        __shared__ unsigned wave_m[ING_THREADS / 64];
        const unsigned m = (__all(all_sc) ? ING_SCALED_OK : 0u) | (__all(all_nm) ? ING_NORMAL_OK : 0u) |
                           (__all(all_fin) ? ING_FINITE : 0u);
        if ((threadIdx.x & 63) == 0) wave_m[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned r = wave_m[0];
#pragma unroll
            for (int i = 1; i < ING_THREADS / 64; i++) r &= wave_m[i];
            if (r != (ING_SCALED_OK | ING_NORMAL_OK | ING_FINITE)) atomicAnd(verdict, r);
        }
    }
}

int ingest_grid(uint64_t words) {
    const uint64_t blocks = (words + ING_THREADS - 1) / ING_THREADS;
    return (int)(blocks < (uint64_t)ING_GRID_CAP ? blocks : (uint64_t)ING_GRID_CAP);
}

}  // namespace

hipError_t launch_ingest_classify(hipStream_t s, const double *X, uint64_t n, uint32_t dim, const double *tab,
                                  unsigned *verdict) {
    static_assert(ING_THREADS == 256, "one thread per table entry");
    const uint32_t wpr = (dim + 3) / 4;
    hipError_t e = hipMemsetAsync(verdict, 0xFF, sizeof(unsigned), s);   // every verdict stands until a workgroup objects
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ingest_kernel<false>, dim3(ingest_grid(n * wpr)), dim3(ING_THREADS), 0, s, X, n, dim, wpr, tab,
                       0u, (uint32_t *)nullptr, verdict);
    return hipGetLastError();
}

hipError_t launch_ingest_pack(hipStream_t s, const double *X, uint64_t n, uint32_t dim, uint32_t cs, const double *tab,
                              uint8_t *codes) {
    const uint32_t wpr = (dim + 3) / 4;
    hipLaunchKernelGGL(ingest_kernel<true>, dim3(ingest_grid(n * wpr)), dim3(ING_THREADS), 0, s, X, n, dim, wpr, tab, cs,
                       reinterpret_cast<uint32_t *>(codes), (unsigned *)nullptr);
    return hipGetLastError();
}

}  // namespace qvq
