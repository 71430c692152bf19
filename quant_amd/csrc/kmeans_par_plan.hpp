// kmeans_par_plan.hpp -- qvq_kmeans_par's options resolved and its launch shape (k_kmeans_par.hip),
// shared by the launchers, the entry point and qvq_host_kmeans_par_plan (engine.cpp).  The row passes
// (update, count, scatter, weights) take kmeanspp_plan's contiguous segments, one block per segment;
// the update holds `chunk` candidates in LDS per trip; the reduction is one block of KMPAR_RED_THREADS
// lanes whose dynamic LDS holds, while they fit, g and wt per candidate and then the candidates' code
// words, all in lane-strided slots (max_candidates rounded up to the block).  Both are decided from
// max_candidates, which the host knows, not from the M a call reaches.
#pragma once
#include <algorithm>
#include <cstdint>

#include "kmeanspp_plan.hpp"

namespace qvq {

constexpr uint32_t KMPAR_THREADS = KMPP_THREADS;   // the row passes: lanes per block
constexpr uint32_t KMPAR_CHUNK = 256;              // candidates the update holds in LDS per trip (<= 2^10: kmpar_pack)
constexpr uint32_t KMPAR_RED_THREADS = 1024;       // the reduction: one block of this many lanes
constexpr uint32_t KMPAR_LDS_BYTES = 160 * 1024;   // a workgroup's LDS
constexpr uint32_t KMPAR_RED_HEAD = 256;           // ... of which the reduction's scan words and broadcasts
constexpr uint32_t KMPAR_ROUNDS_MAX = 16;
constexpr uint32_t KMPAR_K_MAX = 1u << 16, KMPAR_ELL_MAX = 1u << 17, KMPAR_CAND_MAX = 1u << 20;

struct KMeansParPlan {
    uint32_t rounds, ell, round_cap;   // the options, defaults filled in
    uint32_t block, segments, seg_rows;
    uint32_t chunk;
    uint32_t max_candidates;   // 1 + rounds * round_cap
    uint32_t slots;            // max_candidates rounded up to the reduction's lanes: entries of g and of wt
    uint32_t gw_lds;           // the reduction keeps g and wt in LDS (global memory otherwise)
    uint32_t codes_lds;        // ... and the candidates' code words
    uint32_t lds_bytes;        // the reduction's dynamic LDS
};

// 0 = the default.  False: outside the contract's limits (QVQ_EINVAL).
inline bool kmeans_par_options(uint32_t K, uint32_t rounds, uint32_t ell, uint32_t round_cap, KMeansParPlan *p) {
    if (K == 0 || K > KMPAR_K_MAX || rounds > KMPAR_ROUNDS_MAX || ell > KMPAR_ELL_MAX) return false;
    p->rounds = rounds ? rounds : 5;
    p->ell = ell ? ell : K;
    const uint64_t cap = round_cap ? round_cap : 2ull * p->ell + 64;
    if (cap < 1 || 1 + p->rounds * cap > KMPAR_CAND_MAX) return false;
    p->round_cap = (uint32_t)cap;
    p->max_candidates = 1 + p->rounds * p->round_cap;
    return true;
}

// n: 1 .. 2^32 - 1 rows of Dp padded bytes; the options as kmeans_par_options left them.
inline void kmeans_par_shape(uint64_t n, uint32_t Dp, KMeansParPlan *p) {
    const KMeansPPPlan s = kmeanspp_plan(n);
    p->block = KMPAR_THREADS;
    p->segments = s.segments;
    p->seg_rows = s.seg_rows;
    p->chunk = KMPAR_CHUNK;
    p->slots = (p->max_candidates + KMPAR_RED_THREADS - 1) / KMPAR_RED_THREADS * KMPAR_RED_THREADS;
    const uint64_t gw = 8ull * p->slots, codes = (uint64_t)p->slots * Dp;   // a slot per lane and trip
    p->gw_lds = KMPAR_RED_HEAD + gw <= KMPAR_LDS_BYTES;
    p->codes_lds = p->gw_lds && KMPAR_RED_HEAD + gw + codes <= KMPAR_LDS_BYTES;
    p->lds_bytes = KMPAR_RED_HEAD + (p->gw_lds ? (uint32_t)gw : 0) + (p->codes_lds ? (uint32_t)codes : 0);
}

}  // namespace qvq
