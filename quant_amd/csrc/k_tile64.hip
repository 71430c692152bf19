// k_tile64.hip -- rasters straight to exact mode's fp64 rows (qvq_set_images* with QVQ_CS_CIE1931,
// DESIGN.md 3.13), and the byte path's rows as fp64 for qvq_get_vectors.
//
// tile64_kernel tiles n_images rasters exactly as tile_kernel (k_misc.hip) does --
// getBlocksAsVectorsFromImage (src/Compressor.cpp:31-62): block (i, j) of image img is row
// (img * wB + i) * hB + j, its pixel (dx, dy) is raster entry (i * bw + dx) * ySize + (j * bh + dy)
// (columns past ySize run into the next raster row), an entry past the end of its image's buffer is
// three +0.0 -- and writes each pixel through cie1931_from_rgb (cie1931.hpp) into X [N][D], D =
// 3 * bw * bh, no padding: exact mode's d_X64.
//
// The stores are 8x the bytes of the loads, so the kernel is shaped for them: one lane per slot =
// (row, pixel in block), slot s at byte 24 * s, so a wave's three 8-byte stores fill one dense
// 1536-byte run.  Grid-stride over the N * bw * bh slots under T64_GRID_CAP blocks; the lane's
// (image, i, j, dx, dy) is divided out once and then advanced by the stride's digits in the same
// mixed radix (T64Step, worked out by the launcher), a carry per digit and no division in the loop.
// All offsets are 64-bit.
#include "cie1931.hpp"
#include "common.hpp"

namespace qvq {

namespace {

// A slot count in the radices (bh, bw, hB, wB) of the slot order, the images on top.
struct T64Step {
    uint32_t dy, dx, j, i;
    uint64_t img;
};

__host__ __device__ inline T64Step t64_digits(uint64_t s, uint32_t bw, uint32_t bh, uint32_t wB, uint32_t hB) {
    T64Step d;
    d.dy = (uint32_t)(s % bh), s /= bh;
    d.dx = (uint32_t)(s % bw), s /= bw;
    d.j = (uint32_t)(s % hB), s /= hB;
    d.i = (uint32_t)(s % wB), s /= wB;
    d.img = s;
    return d;
}

__global__ void __launch_bounds__(T64_THREADS)
tile64_kernel(const uint8_t *__restrict__ rgb, double *__restrict__ X, uint64_t slots, uint64_t pixels, uint32_t ySize,
              uint32_t bw, uint32_t bh, uint32_t wB, uint32_t hB, T64Step step) {
    const uint64_t stride = (uint64_t)gridDim.x * T64_THREADS;
    uint64_t s = (uint64_t)blockIdx.x * T64_THREADS + threadIdx.x;
    T64Step at = t64_digits(s, bw, bh, wB, hB);
    for (; s < slots; s += stride) {
        const uint64_t px = ((uint64_t)at.i * bw + at.dx) * ySize + ((uint64_t)at.j * bh + at.dy);
        double v[3] = {0.0, 0.0, 0.0};
        if (px < pixels) {
            const uint8_t *p = rgb + (at.img * pixels + px) * 3;
            cie1931_from_rgb((signed char)p[0], (signed char)p[1], (signed char)p[2], v);
        }
        double *o = X + 3 * s;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        // at += step: each digit and its step are below the radix, so one subtraction carries
        uint32_t c;
        at.dy += step.dy, c = at.dy >= bh, at.dy -= c ? bh : 0;
        at.dx += step.dx + c, c = at.dx >= bw, at.dx -= c ? bw : 0;
        at.j += step.j + c, c = at.j >= hB, at.j -= c ? hB : 0;
        at.i += step.i + c, c = at.i >= wB, at.i -= c ? wB : 0;
        at.img += step.img + c;
    }
}

// out [nrows][D] = lut64[codes[row0 + r][d]]: the byte path's rows as the values they stand for, pad
// bytes left out.  One lane per value; (row, d) advances without a division, as above.
__global__ void __launch_bounds__(T64_THREADS)
rows_f64_kernel(const uint8_t *__restrict__ codes, uint32_t Dp, uint32_t D, uint64_t row0, uint64_t nrows,
                const double *__restrict__ lut64, double *__restrict__ out) {
    const uint64_t total = nrows * D;
    const uint64_t stride = (uint64_t)gridDim.x * T64_THREADS;
    uint64_t e = (uint64_t)blockIdx.x * T64_THREADS + threadIdx.x;
    uint64_t row = e / D;
    uint32_t d = (uint32_t)(e % D);
    const uint64_t srow = stride / D;
    const uint32_t sd = (uint32_t)(stride % D);
    for (; e < total; e += stride) {
        out[e] = lut64[codes[(row0 + row) * Dp + d]];
        row += srow;
        d += sd;
        if (d >= D) {
            d -= D;
            row++;
        }
    }
}

int t64_grid(uint64_t lanes) {
    const uint64_t blocks = (lanes + T64_THREADS - 1) / T64_THREADS;
    return (int)(blocks < (uint64_t)T64_GRID_CAP ? blocks : (uint64_t)T64_GRID_CAP);
}

}  // namespace

hipError_t launch_tile64(hipStream_t s, const uint8_t *rgb, double *X, uint32_t n_images, uint32_t xSize,
                         uint32_t ySize, uint32_t bw, uint32_t bh) {
    const uint32_t wB = (xSize + bw - 1) / bw, hB = (ySize + bh - 1) / bh;
    const uint64_t slots = (uint64_t)wB * hB * n_images * bw * bh;
    const int grid = t64_grid(slots);
    const T64Step step = t64_digits((uint64_t)grid * T64_THREADS, bw, bh, wB, hB);
    const uint64_t pixels = (uint64_t)xSize * ySize;
    hipLaunchKernelGGL(tile64_kernel, dim3(grid), dim3(T64_THREADS), 0, s, rgb, X, slots, pixels, ySize, bw, bh, wB, hB,
                       step);
    return hipGetLastError();
}

hipError_t launch_rows_f64(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t row0, uint64_t nrows,
                           const double *lut64, double *out) {
    hipLaunchKernelGGL(rows_f64_kernel, dim3(t64_grid(nrows * D)), dim3(T64_THREADS), 0, s, codes, Dp, D, row0, nrows,
                       lut64, out);
    return hipGetLastError();
}

}  // namespace qvq
