// decode_plan.hpp -- the decode's dispatch (k_misc.hip), shared by launch_decode and by
// qvq_host_decode_plan (engine.cpp): which of the three kernel families a shape and its pointers'
// alignment take, the template arguments, the grid, the dynamic LDS and how often the busiest
// block goes round its grid-stride loop.
#pragma once
#include <algorithm>
#include <cstdint>

namespace qvq {

constexpr uint32_t DEC_THREADS = 256;
// the codebook is staged in LDS up to this many bytes (C3: 12 KB; C4's 196 KB stay in global memory)
constexpr uint32_t DEC_LDS_CB_BYTES = 48 * 1024;
// row kernels with the codebook in LDS: a block loops over several 256-item rounds rather than
// stage the codebook once per round (C3: 8192 one-round blocks staged 100 MB of codebook copies
// for 67 MB of output)
constexpr uint32_t DEC_LDS_GRID_CAP = 2048;
// every other launch: the row kernels without LDS, the per-pixel kernel
constexpr uint32_t DEC_GRID_CAP = 1u << 16;
// COAL: 1536 bytes of staging per wave behind the codebook, 4 waves
constexpr uint32_t DEC_WAVE_STAGE_BYTES = 1536;
constexpr uint32_t DEC_STAGE_BYTES = 4 * DEC_WAVE_STAGE_BYTES;
// the row kernels' byte offsets and item counts are sized for rasters below this many pixels
constexpr uint64_t DEC_ROWS_MAX_PIXELS = 1ull << 40;

enum DecodeKernel : uint32_t { DEC_PIXELS = 0, DEC_ROWS = 1, DEC_ROWS_H = 2 };
// what the caller's pointers lack (0: everything aligned, as the engine's own staging is)
enum : uint32_t {
    DEC_RASTER_UNALIGNED = 1,   // raster % 8 != 0
    DEC_ORIG_UNALIGNED = 2,     // an original is given and original % 8 != 0
    DEC_INDEX_UNALIGNED = 4,    // indices % 16 != 0
    DEC_CODEBOOK_ODD = 8,       // codebook % 2 != 0
};

struct DecodePlan {
    uint32_t kernel;      // DEC_PIXELS: decode_pixels_kernel, DEC_ROWS: decode_rows_kernel<lds>,
                          // DEC_ROWS_H: decode_rows_h_kernel<H, lds, coal>
    uint32_t H;           // ROWS_H: the block height, 1, 2, 4 or 8; 0 otherwise
    uint32_t lds;         // the codebook is staged in LDS
    uint32_t coal;        // ROWS_H: wave-contiguous stores through the LDS staging
    uint32_t grid;        // blocks of DEC_THREADS
    uint32_t lds_bytes;   // dynamic LDS: the codebook rounded up to 16, then the staging
    uint32_t stage_off;   // where the staging starts
    uint64_t rounds;      // trips of the grid-stride loop in block 0
};

// The row kernels store (and read the original) in 8-byte pieces and load 8 / H indices per vector
// load: pointers without that alignment take the per-pixel kernel.  decode_rows_h_kernel reads a
// codebook in global memory through 16-bit loads when H >= 2: an odd codebook pointer then takes
// decode_rows_kernel<false>, which reads bytes (staging into LDS reads bytes as well).
inline DecodePlan decode_plan(uint32_t K, uint32_t xs, uint32_t ys, uint32_t w, uint32_t h, uint32_t unaligned) {
    DecodePlan p{};
    const uint64_t npix = (uint64_t)xs * ys;
    const bool aligned = !(unaligned & (DEC_RASTER_UNALIGNED | DEC_ORIG_UNALIGNED | DEC_INDEX_UNALIGNED));
    uint64_t items;
    if (aligned && ys % 8 == 0 && npix < DEC_ROWS_MAX_PIXELS) {
        items = (uint64_t)xs * (ys / 8);
        const uint64_t cbB = (uint64_t)K * w * h * 3;
        p.lds = cbB <= DEC_LDS_CB_BYTES;
        p.grid = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>((items + DEC_THREADS - 1) / DEC_THREADS, p.lds ? DEC_LDS_GRID_CAP : DEC_GRID_CAP));
        p.lds_bytes = p.lds ? (uint32_t)((cbB + 15) & ~15ull) : 0;
        const bool hset = ys % h == 0 && (h == 1 || h == 2 || h == 4 || h == 8);   // no overhang
        if (hset && (h == 1 || p.lds || !(unaligned & DEC_CODEBOOK_ODD))) {
            p.kernel = DEC_ROWS_H;
            p.H = h;
            // wave-contiguous output chunks need whole waves inside one raster row: 64 | ys / 8
            p.coal = (ys / 8) % 64 == 0;
            p.stage_off = p.lds_bytes;
            if (p.coal) p.lds_bytes += DEC_STAGE_BYTES;
        } else {
            p.kernel = DEC_ROWS;
        }
    } else {
        items = npix;
        p.kernel = DEC_PIXELS;
        p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((npix + DEC_THREADS - 1) / DEC_THREADS, DEC_GRID_CAP));
    }
    const uint64_t per_round = (uint64_t)p.grid * DEC_THREADS;
    p.rounds = (items + per_round - 1) / per_round;
    return p;
}

}  // namespace qvq
