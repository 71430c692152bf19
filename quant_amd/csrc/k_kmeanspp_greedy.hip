// k_kmeanspp_greedy.hip -- qvq_kmeanspp_greedy's rounds (the rule in include/qvq.h, its
// arithmetic in kmeanspp_rule.hpp, the segments kmeanspp_plan()'s, the trial count and the state's
// layout in kmeanspp_greedy_plan.hpp).  Round j draws L candidate rows and keeps the one whose sum of
// min(m, w(., c_l)) is smallest.  A call is
//   init:      the first seed's row (drawn on the host) as round 0's only candidate, the state cleared;
//   evaluate:  a lane per row, block b the rows of segment b.  It applies the previous round's winner,
//              m = min(m, w(row, winner)) stored where it fell, and adds min(m, w(row, c_l)) for each of
//              this round's candidates into part[l][b].  The row is loaded once; the candidates sit in LDS;
//   select:    a block per trial.  Every block sums part[l][.] of the round before (a wave per l) and
//              takes the argmin, lowest l on ties: P of the winner is the potential and this round's T.
//              Block l computes t_l = draw(seed + l 2^32, j, T), finds the segment in the prefix of
//              part[winner][.] (the segment sums of m once the winner is applied) and the row in it by
//              scanning min(m[r], w(r, winner)): the stored m does not hold the winner yet.  It writes
//              candidate l's row and code words.  Block 0 also records the published round.  T = 0:
//              placed = j and the stop flag, on which every later launch returns at once;
// evaluate and select alternate K - 1 times on one stream: two launches a round.  A last select of
// one block only publishes round K - 1.  The candidates' words are double-buffered by round parity:
// the select of round j writes parity j & 1 while the evaluate after it still reads the winner of
// parity (j - 1) & 1.  No block waits on another: the launches are the only ordering.
#include <algorithm>

#include "common.hpp"
#include "kmeanspp_greedy_plan.hpp"
#include "kmeanspp_plan.hpp"
#include "kmeanspp_rule.hpp"

namespace qvq {

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t TR = KMPPG_MAX_TRIALS;
constexpr uint32_t CW = KMPPG_WORDS;
constexpr uint32_t SEL_PER = KMPP_SEGMENTS_CAP / KMPP_SEL_THREADS;   // sums a lane of the select's scan
static_assert(SEL_PER * KMPP_SEL_THREADS == KMPP_SEGMENTS_CAP, "the select takes every sum once");

__device__ inline uint64_t shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, WAVE), hi = __shfl_up((uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_down64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_down((uint32_t)v, d, WAVE), hi = __shfl_down((uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
// the wave's sum, in lane 0
__device__ inline uint64_t wave_sum(uint64_t v) {
    for (uint32_t d = WAVE / 2; d; d >>= 1) v += shfl_down64(v, d);
    return v;
}

// The inclusive prefix of `own` over the block's THREADS lanes in lane order, *total the block's
// sum (the same in every lane).  ws: THREADS / 64 words of LDS, free again on return.
// (k_kmeanspp.hip's block_scan.)
template <uint32_t THREADS>
__device__ inline uint64_t block_scan(uint64_t own, uint64_t *ws, uint64_t *total) {
    constexpr uint32_t WAVES = THREADS / WAVE;
    const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint64_t incl = own;
    for (uint32_t d = 1; d < WAVE; d <<= 1) {
        const uint64_t v = shfl_up64(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane == WAVE - 1) ws[wave] = incl;
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

__global__ __launch_bounds__(WAVE) void kmppg_init_kernel(const uint32_t *__restrict__ codes, uint32_t nw, uint32_t row0,
                                                          uint32_t K, KmppgWork w) {
    const uint32_t i = threadIdx.x;
    if (i == 0) {
        w.state[0] = 0;   // the stop flag
        w.state[1] = K;   // placed, unless a select stops the call
        w.state[2] = 0;
        w.candrow[0] = row0;
    }
    if (i < nw) w.cand[i] = kmpp_ordinals(codes[(uint64_t)row0 * nw + i]);
}

// The row's NW code words as ordinals (k_kmeanspp.hip's load_row).
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

// Round j's evaluate; par = j & 1 is the parity of its candidates.  FIRST (j = 0): the one candidate
// is the first seed and m = w(., s_0) is stored without a read.
template <uint32_t NW, bool FIRST>
__global__ __launch_bounds__(KMPP_THREADS) void kmppg_evaluate_kernel(const uint32_t *__restrict__ codes, uint64_t N,
                                                                      uint32_t seg_rows, uint32_t par, uint32_t L,
                                                                      KmppgWork w) {
    if (w.state[0]) return;   // every row equals a seed already (the same for every thread)
    __shared__ uint32_t sc[TR * NW];   // the candidates' ordinals
    __shared__ uint32_t sn[TR];        // ... and norms
    __shared__ uint64_t ws[KMPP_THREADS / WAVE][TR];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < L * NW; i += KMPP_THREADS) sc[i] = w.cand[(par * TR + i / NW) * CW + i % NW];
    uint32_t wd[NW];   // the previous round's winner
    uint32_t n_win = 0;
    if (!FIRST) {
        const uint32_t *wc = w.cand + ((par ^ 1) * TR + w.state[2]) * CW;
        for (uint32_t i = 0; i < NW; i++) wd[i] = wc[i];
        n_win = kmpp_norm(wd, NW);
    }
    __syncthreads();
    if (tid < L) sn[tid] = kmpp_norm(sc + tid * NW, NW);
    __syncthreads();
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    uint64_t acc[TR];
#pragma unroll
    for (uint32_t l = 0; l < TR; l++) acc[l] = 0;
    for (uint64_t row = row0 + tid; row < end; row += KMPP_THREADS) {
        uint32_t x[NW];
        load_row<NW>(codes, row, x);
        const uint32_t n_x = kmpp_norm(x, NW);
        // the candidates are read from LDS per row (broadcast reads): hoisted out of this loop they
        // would take 17 NW registers a lane and the kernel would run at a third of the occupancy
        asm volatile("" ::: "memory");
        if (FIRST) {
            const uint32_t wgt = kmpp_weight(x, n_x, sc, sn[0], NW);
            w.m[row] = wgt;
            acc[0] += wgt;
        } else {
            uint32_t mv = w.m[row];
            const uint32_t wgt = kmpp_weight(x, n_x, wd, n_win, NW);
            if (wgt < mv) w.m[row] = mv = wgt;
#pragma unroll
            for (uint32_t l = 0; l < TR; l++)
                if (l < L) acc[l] += std::min(mv, kmpp_weight(x, n_x, sc + l * NW, sn[l], NW));
        }
    }
#pragma unroll
    for (uint32_t l = 0; l < TR; l++)
        if (l < L) {
            const uint64_t s = wave_sum(acc[l]);
            if ((tid & (WAVE - 1)) == 0) ws[tid / WAVE][l] = s;
        }
    __syncthreads();
    if (tid < L) {
        uint64_t s = 0;
        for (uint32_t i = 0; i < KMPP_THREADS / WAVE; i++) s += ws[i][tid];
        w.part[(uint64_t)tid * KMPP_SEGMENTS_CAP + blockIdx.x] = s;   // a slot of the block's own
    }
}

// w(r, seed) with the row's words read as they lie; sd holds the seed's ordinals in registers.
__device__ inline uint32_t row_weight(const uint32_t *__restrict__ codes, uint64_t r, uint32_t nw, const uint32_t (&sd)[CW],
                                      uint32_t n_seed) {
    const uint32_t *p = codes + r * nw;
    uint32_t n_x = 0, dot = 0;
#pragma unroll
    for (uint32_t i = 0; i < CW; i++)
        if (i < nw) {
            const uint32_t x = kmpp_ordinals(p[i]);
            n_x = kmpp_dot4(x, x, n_x);
            dot = kmpp_dot4(x, sd[i], dot);
        }
    return n_x + n_seed - 2 * dot;
}

// Select j = 1 .. K - 1 publishes round j - 1 (Lprev candidates) and draws round j's candidate
// blockIdx.x; j = K, one block, only publishes round K - 1.
__global__ __launch_bounds__(KMPP_SEL_THREADS) void kmppg_select_kernel(const uint32_t *__restrict__ codes, uint32_t nw,
                                                                        uint64_t N, uint32_t seg_rows, uint32_t segments,
                                                                        uint32_t j, uint32_t K, uint32_t Lprev, uint64_t seed,
                                                                        KmppgWork w) {
    if (w.state[0]) return;   // (the same for every thread; a block that sees block 0's flag of this launch has T = 0 too)
    __shared__ uint64_t ws[KMPP_SEL_THREADS / WAVE];
    __shared__ uint64_t shP[TR];
    __shared__ uint64_t sh_t;
    __shared__ uint32_t sh_seg;
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (wave < Lprev) {   // P_l of round j - 1: wave l sums part[l][.]
        uint64_t a = 0;
        for (uint32_t s = lane; s < segments; s += WAVE) a += w.part[(uint64_t)wave * KMPP_SEGMENTS_CAP + s];
        a = wave_sum(a);
        if (lane == 0) shP[wave] = a;
    }
    __syncthreads();
    uint32_t win = 0;
    uint64_t T = shP[0];
    for (uint32_t l = 1; l < Lprev; l++) {   // strict: the lowest l wins a tie
        const uint64_t v = shP[l];
        if (v < T) T = v, win = l;
    }
    const uint32_t pp = (j - 1) & 1;
    const uint32_t *wc = w.cand + (pp * TR + win) * CW;   // the winner's ordinals
    if (blockIdx.x == 0) {
        const uint64_t r = j - 1;
        if (tid == 0) {
            w.rows[r] = w.candrow[pp * TR + win];
            w.potential[r] = T;
            w.trial[r] = win;
            w.state[2] = win;
        }
        if (tid < Lprev) {
            w.trial_rows[r * TR + tid] = w.candrow[pp * TR + tid];
            w.trial_potential[r * TR + tid] = shP[tid];
        }
        if (tid < nw) w.seedcodes[r * nw + tid] = kmpp_ordinals(wc[tid]);
    }
    if (j == K) return;
    if (T == 0) {   // every row equals a seed: the call stops at j seeds
        if (blockIdx.x == 0 && tid == 0) w.state[0] = 1, w.state[1] = j;
        return;
    }
    const uint32_t l = blockIdx.x;
    const uint64_t t = kmpp_draw(seed + ((uint64_t)l << 32), j, T);
    // the lowest segment whose inclusive prefix of part[win][.] exceeds t: in exactly one lane's span
    const uint64_t *pw = w.part + (uint64_t)win * KMPP_SEGMENTS_CAP;
    uint64_t p[SEL_PER], own = 0, total;
    for (uint32_t i = 0; i < SEL_PER; i++) {
        const uint32_t s = tid * SEL_PER + i;
        p[i] = s < segments ? pw[s] : 0;
        own += p[i];
    }
    uint64_t incl = block_scan<KMPP_SEL_THREADS>(own, ws, &total);
    if (incl - own <= t && t < incl) {
        uint64_t run = incl - own;
        uint32_t s = tid * SEL_PER;
        for (uint32_t i = 0; i + 1 < SEL_PER && !(t < run + p[i]); i++) run += p[i], s++;
        sh_seg = s;
        sh_t = t - run;
    }
    __syncthreads();
    // the same within the segment's rows, a contiguous run of them per lane, on min(m, w(., winner))
    uint32_t sd[CW];
#pragma unroll
    for (uint32_t i = 0; i < CW; i++) sd[i] = i < nw ? wc[i] : 0;
    const uint32_t n_seed = kmpp_norm(sd, CW);
    const uint64_t base = (uint64_t)sh_seg * seg_rows, len = std::min<uint64_t>(seg_rows, N - base);
    const uint64_t t2 = sh_t, per = (len + KMPP_SEL_THREADS - 1) / KMPP_SEL_THREADS;
    const uint64_t r0 = std::min<uint64_t>(base + len, base + tid * per), r1 = std::min<uint64_t>(base + len, r0 + per);
    own = 0;
    for (uint64_t r = r0; r < r1; r++) own += std::min(w.m[r], row_weight(codes, r, nw, sd, n_seed));
    uint64_t segsum;
    incl = block_scan<KMPP_SEL_THREADS>(own, ws, &segsum);
    if (incl - own <= t2 && t2 < incl) {
        uint64_t run = incl - own, hit = r0;
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t v = std::min(w.m[r], row_weight(codes, r, nw, sd, n_seed));
            if (t2 < run + v) {   // strict: a row with m = 0 is never drawn
                hit = r;
                break;
            }
            run += v;
        }
        const uint32_t slot = (j & 1) * TR + l;
        w.candrow[slot] = (uint32_t)hit;
        for (uint32_t i = 0; i < nw; i++) w.cand[slot * CW + i] = kmpp_ordinals(codes[hit * nw + i]);
    }
}

template <uint32_t NW>
void launch_evaluate_nw(hipStream_t s, const uint32_t *codes, uint64_t N, const KMeansPPPlan &p, uint32_t j, uint32_t L,
                        const KmppgWork &w) {
    if (j == 0)
        hipLaunchKernelGGL((kmppg_evaluate_kernel<NW, true>), dim3(p.segments), dim3(KMPP_THREADS), 0, s, codes, N, p.seg_rows,
                           0u, 1u, w);
    else
        hipLaunchKernelGGL((kmppg_evaluate_kernel<NW, false>), dim3(p.segments), dim3(KMPP_THREADS), 0, s, codes, N, p.seg_rows,
                           j & 1u, L, w);
}

bool bad_shape(const uint8_t *codes, uint32_t Dp, uint64_t N, const KmppgWork &w) {
    return !codes || !w.state || !w.m || N == 0 || N > 0xFFFFFFFFull || Dp == 0 || Dp > 64 || (Dp & 3);
}

}  // namespace

KmppgWork kmppg_work(uint8_t *base, uint32_t *m, uint32_t K, uint32_t Dp) {
    const KmppgLayout l = kmppg_layout(K, Dp);
    KmppgWork w;
    w.state = reinterpret_cast<uint32_t *>(base);
    w.cand = reinterpret_cast<uint32_t *>(base + l.cand);
    w.candrow = reinterpret_cast<uint32_t *>(base + l.candrow);
    w.part = reinterpret_cast<uint64_t *>(base + l.part);
    w.potential = reinterpret_cast<uint64_t *>(base + l.potential);
    w.trial_potential = reinterpret_cast<uint64_t *>(base + l.trial_potential);
    w.rows = reinterpret_cast<uint32_t *>(base + l.rows);
    w.trial = reinterpret_cast<uint32_t *>(base + l.trial);
    w.trial_rows = reinterpret_cast<uint32_t *>(base + l.trial_rows);
    w.seedcodes = reinterpret_cast<uint32_t *>(base + l.seedcodes);
    w.m = m;
    return w;
}

hipError_t launch_kmppg_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                             const KmppgWork &w) {
    if (bad_shape(codes, Dp, N, w) || row0 >= N || K == 0 || K > (1u << 20)) return hipErrorInvalidValue;
    // entries from placed on, and the trials a round did not run: potentials 0, rows and trials 0xFFFFFFFF
    // (potential | trial_potential and rows | trial | trial_rows are adjacent in kmppg_layout)
    hipError_t e = hipMemsetAsync(w.potential, 0, 8ull * K * (1 + TR), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.rows, 0xFF, 4ull * K * (2 + TR), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmppg_init_kernel, dim3(1), dim3(WAVE), 0, s, reinterpret_cast<const uint32_t *>(codes), Dp / 4, row0,
                       K, w);
    return hipGetLastError();
}

hipError_t launch_kmppg_evaluate(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t L,
                                 const KmppgWork &w) {
    if (bad_shape(codes, Dp, N, w) || L == 0 || L > TR) return hipErrorInvalidValue;
    const KMeansPPPlan p = kmeanspp_plan(N);
    const uint32_t *c = reinterpret_cast<const uint32_t *>(codes);
    switch (Dp / 4) {
#define KMPPG_CASE(NW) \
    case NW: launch_evaluate_nw<NW>(s, c, N, p, j, L, w); break;
        KMPPG_CASE(1) KMPPG_CASE(2) KMPPG_CASE(3) KMPPG_CASE(4) KMPPG_CASE(5) KMPPG_CASE(6) KMPPG_CASE(7) KMPPG_CASE(8)
        KMPPG_CASE(9) KMPPG_CASE(10) KMPPG_CASE(11) KMPPG_CASE(12) KMPPG_CASE(13) KMPPG_CASE(14) KMPPG_CASE(15) KMPPG_CASE(16)
#undef KMPPG_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kmppg_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t K,
                               uint32_t L, uint64_t seed, const KmppgWork &w) {
    if (bad_shape(codes, Dp, N, w) || j == 0 || j > K || K > (1u << 20) || L == 0 || L > TR) return hipErrorInvalidValue;
    const KMeansPPPlan p = kmeanspp_plan(N);
    hipLaunchKernelGGL(kmppg_select_kernel, dim3(j == K ? 1 : L), dim3(KMPP_SEL_THREADS), 0, s,
                       reinterpret_cast<const uint32_t *>(codes), Dp / 4, N, p.seg_rows, p.segments, j, K, j == 1 ? 1u : L, seed,
                       w);
    return hipGetLastError();
}

}  // namespace qvq
