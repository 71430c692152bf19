// kmeanspp_greedy_plan.hpp -- qvq_kmeanspp_greedy's trial count and the layout of its device state
// (k_kmeanspp_greedy.hip), shared by the launchers, the entry point and qvq_host_kmpp_trials
// (engine.cpp).  The row segments are kmeanspp_plan()'s, the arithmetic kmeanspp_rule.hpp's.
#pragma once
#include <cstdint>

#include "kmeanspp_plan.hpp"

namespace qvq {

constexpr uint32_t KMPPG_MAX_TRIALS = 16;   // L at most: a wave of the select per trial
static_assert(KMPPG_MAX_TRIALS * 64 == KMPP_SEL_THREADS, "the select sums a trial's segments per wave");
constexpr uint32_t KMPPG_WORDS = 16;        // code words of a candidate's slot (Dp <= 64)

// The trials of a round: `trials` itself in 1 .. 16, and for 0 the default 2 + 7 floor(log2 K) / 10
// (2 at K = 1, 9 at 1024, 16 at 2^20).  false: K or trials outside the call's range.
inline bool kmpp_greedy_trials(uint32_t K, uint32_t trials, uint32_t *L) {
    if (K == 0 || K > (1u << 20) || trials > KMPPG_MAX_TRIALS) return false;
    uint32_t lg = 0;
    while ((K >> lg) > 1) lg++;
    *L = trials ? trials : 2 + 7 * lg / 10;
    return true;
}

// Offsets in bytes into the one allocation that holds all of the call's state but m.  The entries
// that grow with K come last, in the order the results are copied out.
struct KmppgLayout {
    uint64_t cand = 0, candrow = 0, part = 0, potential = 0, rows = 0, trial = 0, trial_rows = 0, trial_potential = 0,
             seedcodes = 0, total = 0;
};
inline KmppgLayout kmppg_layout(uint32_t K, uint32_t Dp) {
    KmppgLayout l;
    uint64_t o = 16;   // state
    l.cand = o, o += 4ull * 2 * KMPPG_MAX_TRIALS * KMPPG_WORDS;
    l.candrow = o, o += 4ull * 2 * KMPPG_MAX_TRIALS;
    l.part = o, o += 8ull * KMPPG_MAX_TRIALS * KMPP_SEGMENTS_CAP;
    l.potential = o, o += 8ull * K;
    l.trial_potential = o, o += 8ull * K * KMPPG_MAX_TRIALS;
    l.rows = o, o += 4ull * K;
    l.trial = o, o += 4ull * K;
    l.trial_rows = o, o += 4ull * K * KMPPG_MAX_TRIALS;
    l.seedcodes = o, o += (uint64_t)K * Dp;
    l.total = o;
    return l;
}

}  // namespace qvq
