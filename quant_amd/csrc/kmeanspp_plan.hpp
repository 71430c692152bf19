// kmeanspp_plan.hpp -- the launch shape of qvq_kmeanspp's update pass (k_kmeanspp.hip), shared by the
// launchers and by qvq_host_kmeanspp_plan (engine.cpp).  The rule needs a prefix of m in row order,
// so the n rows are cut into contiguous segments: block b of the update owns rows
// [b * seg_rows, (b + 1) * seg_rows), a lane per row, and leaves the segment's sum of m in a slot of
// its own.  The segment count is capped, so the select that follows scans the sums in one block.
#pragma once
#include <algorithm>
#include <cstdint>

namespace qvq {

constexpr uint32_t KMPP_THREADS = 256;        // the update: lanes per block
constexpr uint32_t KMPP_SEL_THREADS = 1024;   // the select: one block of this many lanes
// At most this many segments: two sums a lane of the select.  2048 blocks are eight to a CU.
constexpr uint32_t KMPP_SEGMENTS_CAP = 2048;

struct KMeansPPPlan {
    uint32_t block;      // KMPP_THREADS
    uint32_t segments;   // blocks of the update = per-segment sums the select scans
    uint32_t seg_rows;   // rows per segment: a multiple of block, at least one block
};

// n: 1 .. 2^32 - 1 rows.
inline KMeansPPPlan kmeanspp_plan(uint64_t n) {
    KMeansPPPlan p{};
    p.block = KMPP_THREADS;
    const uint64_t per = (n + KMPP_SEGMENTS_CAP - 1) / KMPP_SEGMENTS_CAP;   // rows a segment must take
    const uint64_t seg = std::max<uint64_t>(1, (per + KMPP_THREADS - 1) / KMPP_THREADS) * KMPP_THREADS;
    p.seg_rows = (uint32_t)seg;
    p.segments = (uint32_t)std::max<uint64_t>(1, (n + seg - 1) / seg);
    return p;
}

}  // namespace qvq
