// exact_plan.hpp -- the exact mode's dispatch (k_exact.hip), shared by its launchers and by
// qvq_host_exact_plan / qvq_host_exact_grids (engine.cpp): the LDS budgets, what follows from them
// per dimension, and the grid caps of the grid-stride loops.
#pragma once
#include <cstdint>

namespace qvq {

constexpr int EX_THREADS = 256;
// exact_assign_kernel stages the codebook in LDS in chunks of kc code vectors (kc * D * 8 <=
// EX_LDS_BYTES; one chunk when the codebook fits).
constexpr uint32_t EX_LDS_BYTES = 64 * 1024;
// kahan_chains_lds_kernel: two tile buffers of KC_TILE_BYTES, the 64 KB dynamic LDS default
constexpr uint32_t KC_TILE_BYTES = 32 * 1024;
// blocks of EX_THREADS rows at most; more rows take the kernels' grid-stride loops again
constexpr int EX_ASSIGN_GRID_CAP = 8192;   // exact_assign_kernel
constexpr int EX_IOTA_GRID_CAP = 4096;     // exact_iota_kernel
constexpr int EX_DIST_GRID_CAP = 1024;     // exact_dist_kernel (its partials: EX_DIST_GRID_CAP doubles)

// code vectors per LDS chunk of the search
constexpr uint32_t exact_chunk_codes(uint32_t D) { return EX_LDS_BYTES / (8 * D) ? EX_LDS_BYTES / (8 * D) : 1; }
// rows per LDS tile of the staged Kahan chains
constexpr uint32_t exact_tile_rows(uint32_t D) { return KC_TILE_BYTES / 8 / D; }
// the dimensions of the reference's block shapes: the search holds the row in registers
constexpr bool exact_templated(uint32_t D) { return D == 3 || D == 6 || D == 12 || D == 48; }

}  // namespace qvq
