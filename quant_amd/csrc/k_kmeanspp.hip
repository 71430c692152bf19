// k_kmeanspp.hip -- qvq_kmeanspp's rounds (the rule in include/qvq.h, its
// arithmetic in kmeanspp_rule.hpp, the launch shape in kmeanspp_plan.hpp).  A call is
//   init:    the first seed's row (drawn on the host: it needs no scan), the state cleared;
//   update:  a lane per row, block b the rows of segment b: w(row, seed) from the code words with
//            udot4, m = min(m, w) stored where it fell, the segment's sum of m into partial[b];
//   select:  one block: T = the sum of the partials (published as the previous seed's potential),
//            t = draw(seed, j, T), the segment and then the row whose prefix of m first exceeds t;
//            the row's code words become the next update's seed.  T = 0: placed = j and the stop
//            flag, on which every later launch returns at once;
// update and select alternate K - 1 times on one stream; a last select only publishes the final
// potential.  No block waits on another: the launches are the only ordering.  Integers throughout.
#include <algorithm>

#include "common.hpp"
#include "kmeanspp_plan.hpp"
#include "kmeanspp_rule.hpp"

namespace qvq {

namespace {

constexpr uint32_t KMPP_WAVE = 64;
constexpr uint32_t KMPP_SEL_PER = KMPP_SEGMENTS_CAP / KMPP_SEL_THREADS;   // partials a lane of the select
static_assert(KMPP_SEL_PER * KMPP_SEL_THREADS == KMPP_SEGMENTS_CAP, "the select takes every partial once");

__device__ inline uint64_t shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, KMPP_WAVE), hi = __shfl_up((uint32_t)(v >> 32), d, KMPP_WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_down64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_down((uint32_t)v, d, KMPP_WAVE), hi = __shfl_down((uint32_t)(v >> 32), d, KMPP_WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// The inclusive prefix of `own` over the block's THREADS lanes in lane order, *total the block's
// sum (the same in every lane).  ws: THREADS / 64 words of LDS, free again on return.
template <uint32_t THREADS>
__device__ inline uint64_t block_scan(uint64_t own, uint64_t *ws, uint64_t *total) {
    constexpr uint32_t WAVES = THREADS / KMPP_WAVE;
    const uint32_t lane = threadIdx.x & (KMPP_WAVE - 1), wave = threadIdx.x / KMPP_WAVE;
    uint64_t incl = own;
    for (uint32_t d = 1; d < KMPP_WAVE; d <<= 1) {
        const uint64_t v = shfl_up64(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane == KMPP_WAVE - 1) ws[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t i = 0; i < WAVES; i++) {
        const uint64_t v = ws[i];
        if (i < wave) before += v;
        all += v;
    }
    __syncthreads();
    *total = all;
    return incl + before;
}

__global__ __launch_bounds__(KMPP_WAVE) void kmpp_init_kernel(const uint32_t *__restrict__ codes, uint32_t nw,
                                                              uint32_t row0, uint32_t K, KmppWork w) {
    const uint32_t i = threadIdx.x;
    if (i == 0) {
        w.state[0] = 0;   // the stop flag
        w.state[1] = K;   // placed, unless a select stops the call
        w.rows[0] = row0;
    }
    if (i < nw) {
        const uint32_t word = codes[(uint64_t)row0 * nw + i];
        w.seedw[i] = kmpp_ordinals(word);
        w.seedcodes[i] = word;
    }
}

// The row's NW code words as ordinals.  A row starts at a multiple of 4 NW bytes: rows of 4, 8, 12
// or 16 words are read as 16-byte words, of an even count as 8-byte words.
template <uint32_t NW>
__device__ inline void load_row(const uint32_t *__restrict__ codes, uint64_t row, uint32_t (&x)[NW]) {
    const uint32_t *p = codes + row * NW;
    if constexpr (NW % 4 == 0) {
        for (uint32_t i = 0; i < NW / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            x[4 * i] = v.x, x[4 * i + 1] = v.y, x[4 * i + 2] = v.z, x[4 * i + 3] = v.w;
        }
    } else if constexpr (NW % 2 == 0) {
        for (uint32_t i = 0; i < NW / 2; i++) {
            const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
            x[2 * i] = v.x, x[2 * i + 1] = v.y;
        }
    } else {
        for (uint32_t i = 0; i < NW; i++) x[i] = p[i];
    }
    for (uint32_t i = 0; i < NW; i++) x[i] = kmpp_ordinals(x[i]);
}

// FIRST: the update after the first seed, m = w without a read.
template <uint32_t NW, bool FIRST>
__global__ __launch_bounds__(KMPP_THREADS) void kmpp_update_kernel(const uint32_t *__restrict__ codes, uint64_t N,
                                                                   uint32_t seg_rows, KmppWork w) {
    if (w.state[0]) return;   // every row equals a seed already (the same for every thread)
    __shared__ uint64_t ws[KMPP_THREADS / KMPP_WAVE];
    uint32_t sd[NW];
    for (uint32_t i = 0; i < NW; i++) sd[i] = w.seedw[i];
    const uint32_t n_seed = kmpp_norm(sd, NW);
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    uint64_t acc = 0;
    for (uint64_t row = row0 + threadIdx.x; row < end; row += KMPP_THREADS) {
        uint32_t x[NW];
        load_row<NW>(codes, row, x);
        const uint32_t wgt = kmpp_weight(x, kmpp_norm(x, NW), sd, n_seed, NW);
        uint32_t mv = wgt;
        if (FIRST) {
            w.m[row] = wgt;
        } else {
            mv = w.m[row];
            if (wgt < mv) w.m[row] = mv = wgt;
        }
        acc += mv;
    }
    for (uint32_t d = KMPP_WAVE / 2; d; d >>= 1) acc += shfl_down64(acc, d);
    if ((threadIdx.x & (KMPP_WAVE - 1)) == 0) ws[threadIdx.x / KMPP_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (uint32_t i = 0; i < KMPP_THREADS / KMPP_WAVE; i++) s += ws[i];
        w.partial[blockIdx.x] = s;   // a slot of the block's own
    }
}

// Round j = 1 .. K - 1 places seed j; j = K only publishes the last potential.
__global__ __launch_bounds__(KMPP_SEL_THREADS) void kmpp_select_kernel(const uint32_t *__restrict__ codes, uint32_t nw,
                                                                       uint64_t N, uint32_t seg_rows, uint32_t segments,
                                                                       uint32_t j, uint32_t K, uint64_t seed, KmppWork w) {
    if (w.state[0]) return;   // (the same for every thread)
    __shared__ uint64_t ws[KMPP_SEL_THREADS / KMPP_WAVE];
    __shared__ uint64_t sh_t;
    __shared__ uint32_t sh_seg;
    const uint32_t tid = threadIdx.x;
    uint64_t p[KMPP_SEL_PER], own = 0, T;
    for (uint32_t i = 0; i < KMPP_SEL_PER; i++) {
        const uint32_t s = tid * KMPP_SEL_PER + i;
        p[i] = s < segments ? w.partial[s] : 0;
        own += p[i];
    }
    uint64_t incl = block_scan<KMPP_SEL_THREADS>(own, ws, &T);
    if (tid == 0) w.potential[j - 1] = T;
    if (j == K) return;
    if (T == 0) {   // every row equals a seed: the call stops at j seeds
        if (tid == 0) w.state[0] = 1, w.state[1] = j;
        return;
    }
    const uint64_t t = kmpp_draw(seed, j, T);
    // the lowest segment whose inclusive prefix exceeds t: in exactly one lane's span
    if (incl - own <= t && t < incl) {
        uint64_t run = incl - own;
        uint32_t s = tid * KMPP_SEL_PER;
        for (uint32_t i = 0; i + 1 < KMPP_SEL_PER && !(t < run + p[i]); i++) run += p[i], s++;
        sh_seg = s;
        sh_t = t - run;
    }
    __syncthreads();
    // the same within the segment's rows, a contiguous run of them per lane
    const uint64_t base = (uint64_t)sh_seg * seg_rows, len = std::min<uint64_t>(seg_rows, N - base);
    const uint64_t t2 = sh_t, per = (len + KMPP_SEL_THREADS - 1) / KMPP_SEL_THREADS;
    const uint64_t r0 = std::min<uint64_t>(base + len, base + tid * per), r1 = std::min<uint64_t>(base + len, r0 + per);
    own = 0;
    for (uint64_t r = r0; r < r1; r++) own += w.m[r];
    uint64_t segsum;
    incl = block_scan<KMPP_SEL_THREADS>(own, ws, &segsum);
    if (incl - own <= t2 && t2 < incl) {
        uint64_t run = incl - own, hit = r0;
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t v = w.m[r];
            if (t2 < run + v) {   // strict: a row with m = 0 is never drawn
                hit = r;
                break;
            }
            run += v;
        }
        w.rows[j] = (uint32_t)hit;
        for (uint32_t i = 0; i < nw; i++) {
            const uint32_t word = codes[hit * nw + i];
            w.seedw[i] = kmpp_ordinals(word);
            w.seedcodes[(uint64_t)j * nw + i] = word;
        }
    }
}

template <uint32_t NW>
void launch_update_nw(hipStream_t s, const uint32_t *codes, uint64_t N, const KMeansPPPlan &p, bool first,
                      const KmppWork &w) {
    if (first)
        hipLaunchKernelGGL((kmpp_update_kernel<NW, true>), dim3(p.segments), dim3(KMPP_THREADS), 0, s, codes, N, p.seg_rows, w);
    else
        hipLaunchKernelGGL((kmpp_update_kernel<NW, false>), dim3(p.segments), dim3(KMPP_THREADS), 0, s, codes, N, p.seg_rows, w);
}

bool bad_shape(const uint8_t *codes, uint32_t Dp, uint64_t N, const KmppWork &w) {
    return !codes || !w.state || !w.m || N == 0 || N > 0xFFFFFFFFull || Dp == 0 || Dp > 64 || (Dp & 3);
}

}  // namespace

KmppLayout kmpp_layout(uint32_t K, uint32_t Dp) {
    KmppLayout l;
    uint64_t o = 16;   // state
    l.seedw = o, o += 64;
    l.partial = o, o += 8ull * KMPP_SEGMENTS_CAP;
    l.potential = o, o += 8ull * K;
    l.rows = o, o += 4ull * K;
    l.seedcodes = o, o += (uint64_t)K * Dp;
    l.total = o;
    return l;
}

KmppWork kmpp_work(uint8_t *base, uint32_t *m, uint32_t K, uint32_t Dp) {
    const KmppLayout l = kmpp_layout(K, Dp);
    KmppWork w;
    w.state = reinterpret_cast<uint32_t *>(base);
    w.seedw = reinterpret_cast<uint32_t *>(base + l.seedw);
    w.partial = reinterpret_cast<uint64_t *>(base + l.partial);
    w.potential = reinterpret_cast<uint64_t *>(base + l.potential);
    w.rows = reinterpret_cast<uint32_t *>(base + l.rows);
    w.seedcodes = reinterpret_cast<uint32_t *>(base + l.seedcodes);
    w.m = m;
    return w;
}

hipError_t launch_kmpp_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                            const KmppWork &w) {
    if (bad_shape(codes, Dp, N, w) || row0 >= N || K == 0 || K > (1u << 20)) return hipErrorInvalidValue;
    const KmppLayout l = kmpp_layout(K, Dp);
    uint8_t *base = reinterpret_cast<uint8_t *>(w.state);
    hipError_t e = hipMemsetAsync(base + l.potential, 0, 8ull * K, s);   // entries from placed on repeat 0
    if (e == hipSuccess) e = hipMemsetAsync(base + l.rows, 0xFF, 4ull * K, s);   // ... and hold no row
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmpp_init_kernel, dim3(1), dim3(KMPP_WAVE), 0, s, reinterpret_cast<const uint32_t *>(codes), Dp / 4,
                       row0, K, w);
    return hipGetLastError();
}

hipError_t launch_kmpp_update(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, bool first, const KmppWork &w) {
    if (bad_shape(codes, Dp, N, w)) return hipErrorInvalidValue;
    const KMeansPPPlan p = kmeanspp_plan(N);
    const uint32_t *c = reinterpret_cast<const uint32_t *>(codes);
    switch (Dp / 4) {
#define KMPP_CASE(NW) \
    case NW: launch_update_nw<NW>(s, c, N, p, first, w); break;
        KMPP_CASE(1) KMPP_CASE(2) KMPP_CASE(3) KMPP_CASE(4) KMPP_CASE(5) KMPP_CASE(6) KMPP_CASE(7) KMPP_CASE(8)
        KMPP_CASE(9) KMPP_CASE(10) KMPP_CASE(11) KMPP_CASE(12) KMPP_CASE(13) KMPP_CASE(14) KMPP_CASE(15) KMPP_CASE(16)
#undef KMPP_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kmpp_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t K,
                              uint64_t seed, const KmppWork &w) {
    if (bad_shape(codes, Dp, N, w) || j == 0 || j > K || K > (1u << 20)) return hipErrorInvalidValue;
    const KMeansPPPlan p = kmeanspp_plan(N);
    hipLaunchKernelGGL(kmpp_select_kernel, dim3(1), dim3(KMPP_SEL_THREADS), 0, s, reinterpret_cast<const uint32_t *>(codes),
                       Dp / 4, N, p.seg_rows, p.segments, j, K, seed, w);
    return hipGetLastError();
}

}  // namespace qvq
