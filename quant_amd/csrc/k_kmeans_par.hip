// k_kmeans_par.hip -- qvq_kmeans_par's passes (the rule in include/qvq.h, its
// arithmetic in kmeanspp_rule.hpp and kmeans_par_rule.hpp, the launch shape in kmeans_par_plan.hpp).
// A call is
//   init:     candidate 0's row (drawn on the host), the state cleared;
//   update:   block b the rows of segment b, a lane per row with the row's ordinal words in registers:
//             the round's new candidates pass through LDS in chunks, w(row, c) with udot4, one min per
//             pair on the packed key (weight << 10 | index in the chunk), chunks folded with a strict
//             compare; m and near stored, the segment's sum of m into partial[b];
//   then per round r
//   count:    every block sums the partials itself (phi), a lane per row tests the row, the wave's
//             ballot goes to mask[row / 64], the segment's count to counts[b];
//   scan:     one block: phi published as the previous potential (phi = 0: the stop flag, on which
//             every later round launch returns at once), the counts' exclusive prefix, round_cap
//             applied, the round's candidate range [new_base, new_base + new_cnt) into the state;
//   scatter:  block b places its joining rows in row order from popcounts of the masks: the row and
//             its code words into the candidate list;
//   update:   as above over the new range;
//   weights:  wt[near[row]] += 1, integer atomics;
//   reduce:   one block: the last potential, then weighted k-means++ over the M candidates, the K - 1
//             dependent rounds in one loop: g = min(g, w(., s)) and the lane's sum of wt * g in one
//             pass over the lane's span, a block scan, the draw, the span's lane walks to the
//             candidate.  g, wt and the candidates' code words sit lane-strided in LDS or in global
//             memory, as the plan says; the seed's words are uniform (scalar) data.
// No block waits on another: the launches are the only ordering.  Integers throughout.
#include <algorithm>

#include "common.hpp"
#include "kmeans_par_plan.hpp"
#include "kmeans_par_rule.hpp"

namespace qvq {

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t ROW_WAVES = KMPAR_THREADS / WAVE;
static_assert(KMPAR_CHUNK <= (1u << KMPAR_IDX_BITS) && KMPAR_CHUNK <= KMPAR_THREADS, "a lane fills one candidate of a chunk");
static_assert(KMPP_SEGMENTS_CAP == 2 * KMPAR_RED_THREADS, "the one-block kernels take two segments a lane");

// state words (KmparWork::state)
enum : uint32_t { ST_STOP = 0, ST_M = 1, ST_BASE = 2, ST_CNT = 3, ST_ROUNDS = 4, ST_TRUNC = 5, ST_PLACED = 6, ST_ROUND_CAND = 8 };

__device__ inline uint64_t shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, WAVE), hi = __shfl_up((uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_down64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_down((uint32_t)v, d, WAVE), hi = __shfl_down((uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// The inclusive prefix of `own` over the block's THREADS lanes in lane order, *total the block's sum
// (the same in every lane).  ws: THREADS / 64 words of LDS, free again on return.  (k_kmeanspp.hip's.)
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

// The block's sum of `own`, the same in every lane.  ws as above.
template <uint32_t THREADS>
__device__ inline uint64_t block_sum(uint64_t own, uint64_t *ws) {
    for (uint32_t d = WAVE / 2; d; d >>= 1) own += shfl_down64(own, d);
    if ((threadIdx.x & (WAVE - 1)) == 0) ws[threadIdx.x / WAVE] = own;
    __syncthreads();
    uint64_t s = 0;
    for (uint32_t i = 0; i < THREADS / WAVE; i++) s += ws[i];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(WAVE) void kmpar_init_kernel(const uint32_t *__restrict__ codes, uint32_t nw, uint32_t row0,
                                                          KmparWork w) {
    const uint32_t i = threadIdx.x;
    // 64 words: the flags, the counters and the potentials cleared; candidate 0 is the new range
    w.state[i] = (i == ST_M || i == ST_CNT) ? 1u : 0u;
    if (i == 0) w.cand_rows[0] = row0;
    if (i < nw) w.cand_codes[i] = codes[(uint64_t)row0 * nw + i];
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

// FIRST: the pass after candidate 0, m = w and near = 0 without a read.
template <uint32_t NW, bool FIRST>
__global__ __launch_bounds__(KMPAR_THREADS) void kmpar_update_kernel(const uint32_t *__restrict__ codes, uint64_t N,
                                                                     uint32_t seg_rows, KmparWork w) {
    if (w.state[ST_STOP]) return;   // (the same for every thread)
    const uint32_t base = w.state[ST_BASE], cnt = w.state[ST_CNT];
    if (cnt == 0) return;   // nothing joined: m and the partials stand
    constexpr uint32_t EW = NW + 1;   // a candidate in LDS: norm << 10 | index, then its ordinal words
    __shared__ __attribute__((aligned(16))) uint32_t cand[KMPAR_CHUNK * EW];
    __shared__ uint64_t ws[ROW_WAVES];
    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    uint64_t acc = 0;
    for (uint64_t it0 = row0; it0 < end; it0 += KMPAR_THREADS) {
        const uint64_t row = it0 + tid;
        const bool live = row < end;
        uint32_t x[NW];
        load_row<NW>(codes, live ? row : row0, x);
        const uint32_t nrow = kmpp_norm(x, NW) << KMPAR_IDX_BITS;
        uint32_t mv = 0xFFFFFFFFu, nr = 0;
        if (!FIRST && live) mv = w.m[row], nr = w.near[row];
        for (uint32_t c0 = 0; c0 < cnt; c0 += KMPAR_CHUNK) {
            const uint32_t nc = std::min(KMPAR_CHUNK, cnt - c0);
            __syncthreads();   // the trip before has been read
            if (tid < nc) {
                uint32_t o[NW];
                load_row<NW>(w.cand_codes, base + c0 + tid, o);
                cand[tid * EW] = kmpar_pack(kmpp_norm(o, NW), tid);
                for (uint32_t i = 0; i < NW; i++) cand[tid * EW + 1 + i] = o[i];
            }
            __syncthreads();
            uint32_t best = 0xFFFFFFFFu;
#pragma unroll 4
            for (uint32_t c = 0; c < nc; c++) {
                const uint32_t *e = cand + c * EW;   // the same address in every lane: a broadcast read
                uint32_t dot = 0;
                for (uint32_t i = 0; i < NW; i++) dot = kmpp_dot4(x[i], e[1 + i], dot);
                // (n_row + n_c - 2 dot) << 10 | c: exact, every wrap cancels (the weight is below 2^22)
                best = std::min(best, nrow + e[0] - (dot << (KMPAR_IDX_BITS + 1)));
            }
            const uint32_t wgt = kmpar_key_weight(best);
            if (wgt < mv) mv = wgt, nr = base + c0 + kmpar_key_index(best);   // strict: the lowest index keeps a tie
        }
        if (live) {
            w.m[row] = mv;
            w.near[row] = nr;
            acc += mv;
        }
    }
    const uint64_t s = block_sum<KMPAR_THREADS>(acc, ws);
    if (tid == 0) w.partial[blockIdx.x] = s;   // a slot of the block's own
}

__global__ __launch_bounds__(KMPAR_THREADS) void kmpar_count_kernel(uint64_t N, uint32_t seg_rows, uint32_t segments,
                                                                    uint64_t key, uint32_t ell, KmparWork w) {
    if (w.state[ST_STOP]) return;
    __shared__ uint64_t ws[ROW_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    uint64_t own = 0;
    for (uint32_t s = tid; s < segments; s += KMPAR_THREADS) own += w.partial[s];
    const uint64_t phi = block_sum<KMPAR_THREADS>(own, ws);
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    uint64_t cnt = 0;
    for (uint64_t it0 = row0; it0 < end; it0 += KMPAR_THREADS) {
        const uint64_t row = it0 + tid;
        const bool j = row < end && kmpar_joins(key, row, phi, ell, w.m[row]);
        const uint64_t b = __ballot(j);
        if (lane == 0 && it0 + wave * WAVE < end) {   // (row0 is a multiple of the block: the wave's rows are one word)
            w.mask[(it0 + wave * WAVE) / WAVE] = b;
            cnt += __popcll(b);
        }
    }
    const uint64_t total = block_sum<KMPAR_THREADS>(cnt, ws);
    if (tid == 0) w.counts[blockIdx.x] = (uint32_t)total;
}

// Round r = 1 .. rounds.
__global__ __launch_bounds__(KMPAR_RED_THREADS) void kmpar_scan_kernel(uint32_t segments, uint32_t r, uint32_t round_cap,
                                                                       KmparWork w) {
    if (w.state[ST_STOP]) return;
    __shared__ uint64_t ws[KMPAR_RED_THREADS / WAVE];
    const uint32_t tid = threadIdx.x, s0 = 2 * tid;
    uint64_t phi, total;
    const uint64_t p0 = s0 < segments ? w.partial[s0] : 0, p1 = s0 + 1 < segments ? w.partial[s0 + 1] : 0;
    (void)block_scan<KMPAR_RED_THREADS>(p0 + p1, ws, &phi);
    if (tid == 0) w.potential[r - 1] = phi;
    if (phi == 0) {   // every row equals a candidate: the rounds end
        if (tid == 0) w.state[ST_STOP] = 1;
        return;
    }
    const uint32_t c0 = s0 < segments ? w.counts[s0] : 0, c1 = s0 + 1 < segments ? w.counts[s0 + 1] : 0;
    const uint64_t incl = block_scan<KMPAR_RED_THREADS>((uint64_t)c0 + c1, ws, &total);
    if (s0 < segments) w.offsets[s0] = (uint32_t)(incl - c0 - c1);
    if (s0 + 1 < segments) w.offsets[s0 + 1] = (uint32_t)(incl - c1);
    if (tid == 0) {
        const uint32_t kept = (uint32_t)std::min<uint64_t>(total, round_cap), M = w.state[ST_M];
        if (total > round_cap) w.state[ST_TRUNC] += 1;
        w.state[ST_BASE] = M;
        w.state[ST_CNT] = kept;
        w.state[ST_M] = M + kept;
        w.state[ST_ROUNDS] = r;
        w.state[ST_ROUND_CAND + r - 1] = kept;
    }
}

__global__ __launch_bounds__(KMPAR_THREADS) void kmpar_scatter_kernel(const uint32_t *__restrict__ codes, uint32_t nw,
                                                                      uint64_t N, uint32_t seg_rows, KmparWork w) {
    if (w.state[ST_STOP]) return;
    const uint32_t kept = w.state[ST_CNT], base = w.state[ST_BASE];
    uint32_t running = w.offsets[blockIdx.x];
    if (w.counts[blockIdx.x] == 0 || running >= kept) return;   // none, or all past round_cap
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    for (uint64_t it0 = row0; it0 < end && running < kept; it0 += KMPAR_THREADS) {
        uint32_t before = 0, all = 0;
        uint64_t mine = 0;
        for (uint32_t k = 0; k < ROW_WAVES; k++) {
            const uint64_t b = it0 + k * WAVE < end ? w.mask[(it0 + k * WAVE) / WAVE] : 0;
            const uint32_t n = __popcll(b);
            if (k < wave) before += n;
            if (k == wave) mine = b;
            all += n;
        }
        const uint32_t rank = running + before + __popcll(mine & ((1ull << lane) - 1));
        if (((mine >> lane) & 1) && rank < kept) {   // the round_cap lowest rows are kept
            const uint64_t row = it0 + tid;
            w.cand_rows[base + rank] = (uint32_t)row;
            for (uint32_t i = 0; i < nw; i++) w.cand_codes[(uint64_t)(base + rank) * nw + i] = codes[row * nw + i];
        }
        running += all;
    }
}

__global__ __launch_bounds__(KMPAR_THREADS) void kmpar_weights_kernel(uint64_t N, uint32_t seg_rows, KmparWork w) {
    const uint64_t row0 = (uint64_t)blockIdx.x * seg_rows, end = std::min<uint64_t>(N, row0 + seg_rows);
    for (uint64_t row = row0 + threadIdx.x; row < end; row += KMPAR_THREADS) atomicAdd(&w.cand_wt[w.near[row]], 1u);
}

// A candidate's NW code words at `p` (16-byte aligned when NW % 4 == 0, 8-byte when even) as ordinals.
template <uint32_t NW>
__device__ inline void load_words(const uint32_t *p, uint32_t (&x)[NW]) {
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

// Lane t owns candidates [t * per, (t + 1) * per), so that the prefix in candidate order is a scan
// over the lanes; its i-th candidate's g, wt and code words sit at slot i * lanes + t, so that the
// lanes of a wave read neighbouring memory.
template <uint32_t NW, bool GW_LDS, bool CODES_LDS>
__global__ __launch_bounds__(KMPAR_RED_THREADS) void kmpar_reduce_kernel(uint64_t N, uint32_t segments, uint32_t K,
                                                                         uint64_t seed, uint32_t slots, KmparWork w) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *ws = reinterpret_cast<uint64_t *>(smem);               // [16]
    uint32_t *sh = reinterpret_cast<uint32_t *>(smem + 128);         // [0] the candidate just drawn
    uint32_t *g = GW_LDS ? reinterpret_cast<uint32_t *>(smem + KMPAR_RED_HEAD) : w.gw, *wt = g + slots;
    uint32_t *cw = CODES_LDS ? reinterpret_cast<uint32_t *>(smem + KMPAR_RED_HEAD + 8ull * slots) : w.slotcodes;
    const uint32_t *__restrict__ cc = w.cand_codes;
    const uint32_t tid = threadIdx.x, M = w.state[ST_M];
    if (!w.state[ST_STOP]) {   // the potential after the last round
        uint64_t phi;
        const uint32_t s0 = 2 * tid;
        const uint64_t p0 = s0 < segments ? w.partial[s0] : 0, p1 = s0 + 1 < segments ? w.partial[s0 + 1] : 0;
        (void)block_scan<KMPAR_RED_THREADS>(p0 + p1, ws, &phi);
        if (tid == 0) w.potential[w.state[ST_ROUNDS]] = phi;
    }
    const uint32_t per = (M + KMPAR_RED_THREADS - 1) / KMPAR_RED_THREADS;
    const uint32_t cb = std::min(M, tid * per), ce = std::min(M, cb + per);
    uint64_t own = 0, total;
    for (uint32_t c = cb; c < ce; c++) {   // once: the lane's candidates into their slots
        const uint32_t slot = (c - cb) * KMPAR_RED_THREADS + tid, v = w.cand_wt[c];
        wt[slot] = v;
        own += v;
        for (uint32_t i = 0; i < NW; i++) cw[(uint64_t)slot * NW + i] = cc[(uint64_t)c * NW + i];
    }
    const uint64_t rseed = kmpar_reduce_seed(seed);
    uint64_t incl = block_scan<KMPAR_RED_THREADS>(own, ws, &total);   // total = N
    uint64_t t = kmpp_draw(rseed, 0, total);
    if (incl - own <= t && t < incl) {
        uint64_t run = incl - own;
        uint32_t hit = cb;
        for (uint32_t c = cb; c < ce; c++) {
            const uint64_t v = wt[(c - cb) * KMPAR_RED_THREADS + tid];
            if (t < run + v) {   // strict: a candidate of weight 0 is never drawn
                hit = c;
                break;
            }
            run += v;
        }
        sh[0] = hit;
    }
    __syncthreads();
    uint32_t placed = K;
    for (uint32_t j = 0;; j++) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(sh[0]);   // the same in every lane
        uint32_t sd[NW];
        for (uint32_t i = 0; i < NW; i++) sd[i] = cc[(uint64_t)s * NW + i];   // as stored: the seed's code words
        if (tid == 0) w.rows[j] = w.cand_rows[s];
        if (tid < NW) w.seedcodes[(uint64_t)j * NW + tid] = cc[(uint64_t)s * NW + tid];
        if (j + 1 == K) break;
        for (uint32_t i = 0; i < NW; i++) sd[i] = kmpp_ordinals(sd[i]);
        const uint32_t n_seed = kmpp_norm(sd, NW);
        own = 0;
        for (uint32_t c = cb; c < ce; c++) {
            const uint32_t slot = (c - cb) * KMPAR_RED_THREADS + tid;
            uint32_t x[NW];
            load_words<NW>(cw + (uint64_t)slot * NW, x);
            uint32_t gv = kmpp_weight(x, kmpp_norm(x, NW), sd, n_seed, NW);
            if (j) gv = std::min(gv, g[slot]);
            g[slot] = gv;
            own += (uint64_t)wt[slot] * gv;
        }
        incl = block_scan<KMPAR_RED_THREADS>(own, ws, &total);
        if (total == 0) {   // every candidate of weight > 0 equals a seed
            placed = j + 1;
            break;
        }
        t = kmpp_draw(rseed, j + 1, total);
        if (incl - own <= t && t < incl) {
            uint64_t run = incl - own;
            uint32_t hit = cb;
            for (uint32_t c = cb; c < ce; c++) {
                const uint32_t slot = (c - cb) * KMPAR_RED_THREADS + tid;
                const uint64_t v = (uint64_t)wt[slot] * g[slot];
                if (t < run + v) {
                    hit = c;
                    break;
                }
                run += v;
            }
            sh[0] = hit;
        }
        __syncthreads();
    }
    if (tid == 0) w.state[ST_PLACED] = placed;
}

bool bad_shape(const uint8_t *codes, uint32_t Dp, uint64_t N, const KmparWork &w) {
    return !codes || !w.state || !w.m || !w.near || !w.mask || N == 0 || N > 0xFFFFFFFFull || Dp == 0 || Dp > 64 || (Dp & 3);
}

template <uint32_t NW>
void launch_update_nw(hipStream_t s, const uint32_t *codes, uint64_t N, const KMeansParPlan &p, bool first,
                      const KmparWork &w) {
    if (first)
        hipLaunchKernelGGL((kmpar_update_kernel<NW, true>), dim3(p.segments), dim3(KMPAR_THREADS), 0, s, codes, N, p.seg_rows, w);
    else
        hipLaunchKernelGGL((kmpar_update_kernel<NW, false>), dim3(p.segments), dim3(KMPAR_THREADS), 0, s, codes, N, p.seg_rows, w);
}

}  // namespace

KmparLayout kmpar_layout(uint32_t K, uint32_t Dp, const KMeansParPlan &p) {
    KmparLayout l;
    const uint64_t mc = p.max_candidates;
    uint64_t o = 256;   // state
    l.partial = o, o += 8ull * KMPP_SEGMENTS_CAP;
    l.counts = o, o += 4ull * KMPP_SEGMENTS_CAP;
    l.offsets = o, o += 4ull * KMPP_SEGMENTS_CAP;
    l.cand_rows = o, o += 4 * mc;
    l.cand_wt = o, o += 4 * mc;
    l.rows = o, o += 4ull * K;
    o = (o + 15) & ~15ull;
    l.cand_codes = o, o += mc * Dp;
    o = (o + 15) & ~15ull;
    l.seedcodes = o, o += (uint64_t)K * Dp;
    o = (o + 15) & ~15ull;
    l.gw = o, o += 8ull * p.slots;
    l.slotcodes = o, o += p.codes_lds ? 0 : (uint64_t)p.slots * Dp;
    l.total = o;
    return l;
}

KmparWork kmpar_work(uint8_t *base, uint32_t *m, uint32_t *near, uint64_t *mask, const KmparLayout &l) {
    KmparWork w;
    w.state = reinterpret_cast<uint32_t *>(base);
    w.potential = reinterpret_cast<uint64_t *>(base + 96);
    w.partial = reinterpret_cast<uint64_t *>(base + l.partial);
    w.counts = reinterpret_cast<uint32_t *>(base + l.counts);
    w.offsets = reinterpret_cast<uint32_t *>(base + l.offsets);
    w.cand_rows = reinterpret_cast<uint32_t *>(base + l.cand_rows);
    w.cand_wt = reinterpret_cast<uint32_t *>(base + l.cand_wt);
    w.rows = reinterpret_cast<uint32_t *>(base + l.rows);
    w.cand_codes = reinterpret_cast<uint32_t *>(base + l.cand_codes);
    w.seedcodes = reinterpret_cast<uint32_t *>(base + l.seedcodes);
    w.gw = reinterpret_cast<uint32_t *>(base + l.gw);
    w.slotcodes = reinterpret_cast<uint32_t *>(base + l.slotcodes);
    w.m = m, w.near = near, w.mask = mask;
    return w;
}

hipError_t launch_kmpar_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                             const KMeansParPlan &p, const KmparLayout &l, const KmparWork &w) {
    if (bad_shape(codes, Dp, N, w) || row0 >= N || K == 0 || K > KMPAR_K_MAX) return hipErrorInvalidValue;
    uint8_t *base = reinterpret_cast<uint8_t *>(w.state);
    // cand_rows | cand_wt | rows are adjacent: entries from M on hold no row and weight 0, rows from placed on no row
    hipError_t e = hipMemsetAsync(base + l.cand_rows, 0xFF, 4ull * p.max_candidates, s);
    if (e == hipSuccess) e = hipMemsetAsync(base + l.cand_wt, 0, 4ull * p.max_candidates, s);
    if (e == hipSuccess) e = hipMemsetAsync(base + l.rows, 0xFF, 4ull * K, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmpar_init_kernel, dim3(1), dim3(WAVE), 0, s, reinterpret_cast<const uint32_t *>(codes), Dp / 4, row0, w);
    return hipGetLastError();
}

hipError_t launch_kmpar_update(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               bool first, const KmparWork &w) {
    if (bad_shape(codes, Dp, N, w)) return hipErrorInvalidValue;
    const uint32_t *c = reinterpret_cast<const uint32_t *>(codes);
    switch (Dp / 4) {
#define KMPAR_CASE(NW) \
    case NW: launch_update_nw<NW>(s, c, N, p, first, w); break;
        KMPAR_CASE(1) KMPAR_CASE(2) KMPAR_CASE(3) KMPAR_CASE(4) KMPAR_CASE(5) KMPAR_CASE(6) KMPAR_CASE(7) KMPAR_CASE(8)
        KMPAR_CASE(9) KMPAR_CASE(10) KMPAR_CASE(11) KMPAR_CASE(12) KMPAR_CASE(13) KMPAR_CASE(14) KMPAR_CASE(15) KMPAR_CASE(16)
#undef KMPAR_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kmpar_sample(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               uint32_t r, uint64_t seed, const KmparWork &w) {
    if (bad_shape(codes, Dp, N, w) || r == 0 || r > p.rounds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmpar_count_kernel, dim3(p.segments), dim3(KMPAR_THREADS), 0, s, N, p.seg_rows, p.segments,
                       kmpar_round_key(seed, r), p.ell, w);
    hipLaunchKernelGGL(kmpar_scan_kernel, dim3(1), dim3(KMPAR_RED_THREADS), 0, s, p.segments, r, p.round_cap, w);
    hipLaunchKernelGGL(kmpar_scatter_kernel, dim3(p.segments), dim3(KMPAR_THREADS), 0, s,
                       reinterpret_cast<const uint32_t *>(codes), Dp / 4, N, p.seg_rows, w);
    return hipGetLastError();
}

hipError_t launch_kmpar_weights(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                                const KmparWork &w) {
    if (bad_shape(codes, Dp, N, w)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmpar_weights_kernel, dim3(p.segments), dim3(KMPAR_THREADS), 0, s, N, p.seg_rows, w);
    return hipGetLastError();
}

template <uint32_t NW>
static void launch_reduce_nw(hipStream_t s, uint64_t N, const KMeansParPlan &p, uint32_t K, uint64_t seed, const KmparWork &w) {
    const dim3 grid(1), block(KMPAR_RED_THREADS);
    if (p.codes_lds)
        hipLaunchKernelGGL((kmpar_reduce_kernel<NW, true, true>), grid, block, p.lds_bytes, s, N, p.segments, K, seed, p.slots, w);
    else if (p.gw_lds)
        hipLaunchKernelGGL((kmpar_reduce_kernel<NW, true, false>), grid, block, p.lds_bytes, s, N, p.segments, K, seed, p.slots, w);
    else
        hipLaunchKernelGGL((kmpar_reduce_kernel<NW, false, false>), grid, block, p.lds_bytes, s, N, p.segments, K, seed, p.slots, w);
}

hipError_t launch_kmpar_reduce(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               uint32_t K, uint64_t seed, const KmparWork &w) {
    if (bad_shape(codes, Dp, N, w) || K == 0 || K > KMPAR_K_MAX || p.lds_bytes > KMPAR_LDS_BYTES) return hipErrorInvalidValue;
    switch (Dp / 4) {
#define KMPAR_CASE(NW) \
    case NW: launch_reduce_nw<NW>(s, N, p, K, seed, w); break;
        KMPAR_CASE(1) KMPAR_CASE(2) KMPAR_CASE(3) KMPAR_CASE(4) KMPAR_CASE(5) KMPAR_CASE(6) KMPAR_CASE(7) KMPAR_CASE(8)
        KMPAR_CASE(9) KMPAR_CASE(10) KMPAR_CASE(11) KMPAR_CASE(12) KMPAR_CASE(13) KMPAR_CASE(14) KMPAR_CASE(15) KMPAR_CASE(16)
#undef KMPAR_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace qvq
