// mean_plan.hpp -- the launch shape of the K = 1 sums (mean_sums_kernel, k_misc.hip), shared by
// launch_mean_sums and by qvq_host_mean_grid (engine.cpp).  The kernel adds every component's exact
// term in 16-bit register fields (u = b ^ 0x80 <= 255 in one, lo8[b] <= 128 in the other), so a
// field holds MEAN_FIELD_ADDS = 257 adds (255 * 257 = 65535) and no more.  Nothing in the kernel
// counts them: this grid is what keeps every thread within that many.
//
// Who adds what (the kernel's three loops, in groups of MEAN_GROUP_ROWS = 4 consecutive rows):
//   1. Dp <= 16 only: chunks of MEAN_CHUNK_GROUPS = 64 groups, chunk c to wave c mod nwaves (nwaves
//      = 16 * grid).  A chunk is 4 adds to every field of every lane of its wave.  Wave 0 of block 0
//      takes the most, ceil(chunks / nwaves).
//   2. the groups left (fewer than 64 after the chunks; every group where Dp > 16), group g to
//      thread g mod (1024 * grid): 4 adds.  After the chunks these are threads 0 .. 62 of block 0:
//      lanes of that same wave 0.
//   3. the last N mod 4 rows, one each to threads 0 .. 2 of block 0: 1 add.
// So thread 0 of block 0 makes 4 * ceil(chunks / nwaves) + 4 [a group is left] + 1 [N mod 4 != 0]
// adds (Dp > 16: 4 * ceil(groups / (1024 * grid)) + 1), and no thread makes more.
#pragma once
#include <algorithm>
#include <cstdint>

namespace qvq {

constexpr int MEAN_THREADS = 1024;
constexpr uint64_t MEAN_ROWS_PER_THREAD = 256;
constexpr int MEAN_U = 4;                    // chunks (Dp <= 16: also groups) in flight per trip
constexpr uint32_t MEAN_GROUP_ROWS = 4;      // rows per group: Dp / 4 16-byte loads
constexpr uint32_t MEAN_CHUNK_GROUPS = 64;   // groups per wave chunk: one per lane
constexpr uint32_t MEAN_GRID_CAP = 256;      // one block per CU while every thread stays within its fields
constexpr uint32_t MEAN_FIELD_ADDS = 257;    // adds of 255 a 16-bit field holds

__host__ __device__ constexpr bool mean_chunk_loop(int Dp) { return Dp <= 16; }
// groups in flight per trip of the per-thread loop (wide rows: fewer, by registers)
__host__ __device__ constexpr int mean_groups_in_flight(int Dp) { return Dp <= 16 ? MEAN_U : (Dp <= 32 ? 2 : 1); }

struct MeanPlan {
    uint64_t grid;               // summing blocks (the launch adds one block that only initialises)
    uint32_t threads;            // MEAN_THREADS
    uint32_t group_rows;         // MEAN_GROUP_ROWS
    uint32_t chunk_groups;       // MEAN_CHUNK_GROUPS
    uint32_t chunks_in_flight;   // MEAN_U
    uint32_t groups_in_flight;   // mean_groups_in_flight(Dp)
    uint32_t chunk_loop;         // 1: loop 1 runs (Dp <= 16)
};

// N rows of Dp (a multiple of 4, at most 64) code bytes.
inline MeanPlan mean_plan(uint64_t N, uint32_t Dp) {
    MeanPlan p{};
    p.threads = MEAN_THREADS;
    p.group_rows = MEAN_GROUP_ROWS;
    p.chunk_groups = MEAN_CHUNK_GROUPS;
    p.chunks_in_flight = MEAN_U;
    p.groups_in_flight = (uint32_t)mean_groups_in_flight((int)Dp);
    p.chunk_loop = mean_chunk_loop((int)Dp);
    // one block per CU (few same-address atomics at the end), more only where a thread would
    // otherwise take over MEAN_ROWS_PER_THREAD rows
    const uint64_t per_block = MEAN_THREADS * MEAN_ROWS_PER_THREAD;
    const uint64_t grid_rows = (N + per_block - 1) / per_block;
    uint64_t grid = std::max<uint64_t>(std::max<uint64_t>(grid_rows, 1),
                                       std::min<uint64_t>((N + 4 * MEAN_THREADS - 1) / (4 * MEAN_THREADS), MEAN_GRID_CAP));
    if (p.chunk_loop) {
        // Rows per thread are an average: wave 0 rounds its share of the chunks up and then takes
        // the leftover group and a tail row on top (261 adds at N = 2^26 - 249 on 256 blocks, where
        // the average is under 256).  Its chunks are capped so that the three loops together stay
        // within MEAN_FIELD_ADDS: 64 chunks (256 adds, 257 with a tail row), 63 when a group is
        // left (252 + 4 + 1).  Binds from N = 66 060 548 rows; below that the grid is the one above.
        const uint64_t groups = N / MEAN_GROUP_ROWS;
        const uint64_t chunks = groups / MEAN_CHUNK_GROUPS;
        const uint64_t spare = MEAN_FIELD_ADDS - 1 - (groups % MEAN_CHUNK_GROUPS ? MEAN_GROUP_ROWS : 0);
        const uint64_t wave_chunks = spare / MEAN_GROUP_ROWS * (MEAN_THREADS / 64);   // per block
        grid = std::max<uint64_t>(grid, (chunks + wave_chunks - 1) / wave_chunks);
    }
    // (Dp > 16: thread 0 takes ceil(groups / (1024 grid)) <= 64 groups and a tail row, 257 adds at most)
    p.grid = grid;   // N < 2^32: under 2^15 blocks
    return p;
}

}  // namespace qvq
