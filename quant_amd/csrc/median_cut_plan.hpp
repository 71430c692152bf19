// median_cut_plan.hpp -- the dispatch of one median-cut level (k_mediancut.hip), shared by the
// launchers and by qvq_host_median_cut_plan (engine.cpp): which variant each of the level's two row
// passes takes for `boxes` boxes of `dim` components, and the passes' launch shape for n rows.
#pragma once
#include <algorithm>
#include <cstdint>

namespace qvq {

constexpr uint32_t MC_THREADS = 256;      // both row passes: a lane per row
constexpr uint32_t MC_GRID_CAP = 768;     // at most this many blocks: more rows take the grid-stride loop again
// the per-box state a block privatises in LDS, in 32-bit words (48 KB: three blocks to a CU)
constexpr uint32_t MC_LDS_WORDS = 12288;
// More boxes than a block's LDS holds are cut into groups of boxes that fit: a group's blocks read
// every row's label (4 bytes) and take the rows of their boxes only.  Past this many groups the
// label reads cost more than they save (the boxes then hold few rows each): global atomics.
constexpr uint32_t MC_MAX_GROUPS = 16;

struct MedianCutPlan {
    uint32_t range_lds;    // ranges pass: the boxes' minima and maxima are privatised in LDS
    uint32_t hist_lds;     // histogram pass: the boxes' 256 bins are privatised in LDS
    uint32_t full_hist;    // the per-(box, dim) histograms in one pass: not taken by this build (0)
    uint32_t block;        // lanes per block, both passes
    uint32_t range_cap, hist_cap;     // the passes' grid caps per group, in blocks
    uint32_t range_grid, hist_grid;   // blocks per group launched for n rows
    uint32_t lds_words;    // MC_LDS_WORDS
    uint32_t range_groups, hist_groups;         // groups of boxes (1: every box in one block's LDS; 0: not in LDS)
    uint32_t range_group_boxes, hist_group_boxes;   // boxes per group
};

inline uint32_t mc_grid(uint64_t n, uint32_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + MC_THREADS - 1) / MC_THREADS, cap));
}
// The largest power of two of boxes, at most `boxes`, whose `per_box` words each fit the LDS.
inline uint32_t mc_group_boxes(uint32_t boxes, uint32_t per_box) {
    uint32_t g = 1;
    while (2 * g <= boxes && 2ull * g * per_box <= MC_LDS_WORDS) g *= 2;
    return g;
}

// boxes: a power of two (the level's 2^(l-1)).
inline MedianCutPlan median_cut_plan(uint32_t dim, uint32_t boxes, uint64_t n) {
    MedianCutPlan p{};
    p.block = MC_THREADS;
    p.lds_words = MC_LDS_WORDS;
    p.full_hist = 0;
    p.range_group_boxes = mc_group_boxes(boxes, 2 * dim);
    p.hist_group_boxes = mc_group_boxes(boxes, 256);
    const uint32_t rg = boxes / p.range_group_boxes, hg = boxes / p.hist_group_boxes;
    // (a group of the ranges pass is the two children of each of its parents: at least two boxes)
    p.range_lds = rg <= MC_MAX_GROUPS && (boxes == 1 || p.range_group_boxes >= 2);
    p.hist_lds = hg <= MC_MAX_GROUPS;
    p.range_groups = p.range_lds ? rg : 0;
    p.hist_groups = p.hist_lds ? hg : 0;
    p.range_cap = MC_GRID_CAP / std::max<uint32_t>(1, p.range_groups);
    p.hist_cap = MC_GRID_CAP / std::max<uint32_t>(1, p.hist_groups);
    p.range_grid = mc_grid(n, p.range_cap);
    p.hist_grid = mc_grid(n, p.hist_cap);
    return p;
}

}  // namespace qvq
