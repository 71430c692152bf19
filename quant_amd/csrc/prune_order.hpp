// prune_order.hpp -- the pruned searches' code-vector order (device code of the finalize kernel,
// k_finalize.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfma_util.hpp"

namespace qvq {

// The next search's code-vector order for tile pruning (assign_mf32_kernel / assign_wide_kernel
// PRUNE): the K2 split code vectors bucket-sorted by their projection q = sum_d (c_d - mu) / sx on
// the all-ones direction (in the units of a row's sum_d w_d, w the centred byte integers), so that
// each 32-code-vector tile spans a short q interval.  perm[p] = the code vector at position p
// (padding positions K2 .. Kpad map to themselves); tint[2t], tint[2t + 1] = tile t's envelope:
// the floor / ceil of its q interval widened by 1 (empty tile: INT_MAX, INT_MIN), then the suffix
// minimum of the lows and the prefix maximum of the highs.  Any grouping keeps the search exact
// (the bound holds for every tile); the sort only makes it prune.  Run by the finalize's last
// block (any size >= 256: threads past 256 only meet the barriers), K2 <= PRUNE_MAXK.
constexpr uint32_t PRUNE_MAXK = 4096, PRUNE_NB = 256, PRUNE_MAXT = PRUNE_MAXK / 32;
__device__ void prune_order(const float *__restrict__ qproj, uint32_t K2, uint32_t Kpad, uint32_t *__restrict__ perm,
                            int32_t *__restrict__ tint) {
    __shared__ float q[PRUNE_MAXK];
    __shared__ float qs[PRUNE_MAXK];   // q by position
    __shared__ uint32_t hist[PRUNE_NB];
    __shared__ int32_t tlo[PRUNE_MAXT], thi[PRUNE_MAXT];
    __shared__ uint32_t wtot[4], wlo[4], whi[4];
    const uint32_t tid = threadIdx.x;
    const bool act = tid < 256;
    float mn = INFINITY, mx = -INFINITY;
    for (uint32_t j = tid; act && j < K2; j += 256) {   // (the finalize items wrote them)
        q[j] = __builtin_nontemporal_load(&qproj[j]);
        mn = fminf(mn, q[j]);
        mx = fmaxf(mx, q[j]);
    }
    // the range of q: DPP wave minima of the floats as order-preserving u32, then the four waves'
    auto ford = [](float f) {
        const uint32_t b = __float_as_uint(f);
        return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    };
    auto fdec = [](uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); };
    const uint32_t umn = wave_min_u32(ford(mn)), umx = ~wave_min_u32(~ford(mx));
    if (act) {
        hist[tid] = 0;
        if ((tid & 63) == 0) {
            wlo[tid >> 6] = umn;
            whi[tid >> 6] = umx;
        }
    }
    __syncthreads();
    const float qmin = fdec(min(min(wlo[0], wlo[1]), min(wlo[2], wlo[3])));
    const float qmax = fdec(max(max(whi[0], whi[1]), max(whi[2], whi[3])));
    const float inv = (float)PRUNE_NB / (qmax - qmin + 1.0f);
    auto bucket = [&](float v) { return min((uint32_t)((v - qmin) * inv), PRUNE_NB - 1); };
    if (act)
        for (uint32_t j = tid; j < K2; j += 256) atomicAdd(&hist[bucket(q[j])], 1u);
    __syncthreads();
    {   // exclusive scan of the 256 bucket counts (one per thread): DPP scans within the four
        // waves, then each wave adds the totals of the waves before it (two barriers, not 16)
        static_assert(PRUNE_NB == 256, "one bucket per thread");
        const uint32_t own = act ? hist[tid] : 0u;
        const uint32_t inc = wave_scan_add(own);
        if (act && (tid & 63) == 63) wtot[tid >> 6] = inc;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t w = 0; act && w < (tid >> 6); w++) pre += wtot[w];
        if (act) hist[tid] = pre + inc - own;
    }
    __syncthreads();
    if (act) {
        for (uint32_t j = tid; j < K2; j += 256) {   // (order inside a bucket: any)
            const uint32_t p = atomicAdd(&hist[bucket(q[j])], 1u);
            perm[p] = j;
            qs[p] = q[j];
        }
        for (uint32_t p = K2 + tid; p < Kpad; p += 256) perm[p] = p;
    }
    __syncthreads();
    // tile t = positions 32t .. 32t + 31: thread t < nt scans its tile
    const uint32_t nt = Kpad / 32;
    if (act && tid < nt) {
        float lo = INFINITY, hi = -INFINITY;
        for (uint32_t p = 32 * tid; p < min(32 * tid + 32, K2); p++) {
            lo = fminf(lo, qs[p]);
            hi = fmaxf(hi, qs[p]);
        }
        tlo[tid] = lo <= hi ? (int32_t)floorf(lo) - 1 : 0x7FFFFFFF;
        thi[tid] = lo <= hi ? (int32_t)ceilf(hi) + 1 : (int32_t)0x80000000;
    }
    // Tiles sharing a bucket can overlap out of order: monotone envelopes (lo: the suffix
    // minimum, hi: the prefix maximum; still bounds of every tile), so that the tiles a bound
    // admits form one contiguous range.  DPP max-scans over nt <= 128 entries in two waves (the
    // lows in reversed tile order, mapped so that a smaller int is a larger u32; 0 is the
    // neutral value of both maps, as INT_MAX / INT_MIN are of the envelopes).
    __syncthreads();
    const int r = (int)nt - 1 - (int)tid;   // this thread's tile for the suffix scan
    uint32_t hm = act && tid < nt ? (uint32_t)thi[tid] ^ 0x80000000u : 0u;
    uint32_t lm = act && r >= 0 ? ~((uint32_t)tlo[r] ^ 0x80000000u) : 0u;
    hm = wave_scan_max(hm);
    lm = wave_scan_max(lm);
    if (act && (tid & 63) == 63) {
        whi[tid >> 6] = hm;
        wlo[tid >> 6] = lm;
    }
    __syncthreads();
    for (uint32_t w = 0; act && w < (tid >> 6); w++) {
        hm = max(hm, whi[w]);
        lm = max(lm, wlo[w]);
    }
    if (act && tid < nt) tint[2 * tid + 1] = (int32_t)(hm ^ 0x80000000u);
    if (act && r >= 0) tint[2 * r] = (int32_t)(~lm ^ 0x80000000u);
}

}  // namespace qvq
