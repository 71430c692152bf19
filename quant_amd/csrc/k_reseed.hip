// k_reseed.hip -- qvq_refine's empty-cell reseed (QVQ_REFINE_RESEED; DESIGN.md 3.11, the rule in
// reseed_rule.hpp): three launches between an iteration's centroid step and its tables.
//   count:  the cells' row counts from the reduced sums, the number of empty cells, E and far cleared;
//   rows:   every row's quantised error against its cell's centroid: E_k += q (u64 integer adds, so
//           the order does not matter), far_k = max (q << 32 | ~row);
//   select: empties in ascending k, donors by (E desc, k asc), the seeds written into the codebook,
//           the count published.
// The rows pass and the select return at once when the count found no empty cell.
#include <algorithm>

#include "common.hpp"
#include "reseed_rule.hpp"

namespace qvq {

namespace {

constexpr uint32_t RSD_LDS_K = 2048;     // rows pass: cells privatised in LDS (16 B each: 32 KB)
constexpr int RSD_SEL_THREADS = 1024;    // the select: one block
constexpr uint32_t RSD_SEL_LDS = 2048;   // donors sorted in LDS (12 B each: 24 KB), more in global memory

typedef unsigned long long ull;

__global__ __launch_bounds__(RSD_THREADS) void reseed_count_kernel(const uint64_t *__restrict__ sums, uint32_t K,
                                                                   uint32_t D, uint32_t ncopy, uint64_t cstride,
                                                                   const unsigned *__restrict__ gate, ReseedWork w) {
    __shared__ unsigned wsum[RSD_THREADS / 64];
    const uint64_t cnt0 = 2ull * K * D;
    // (the finalize's gate: without ties the further copies are all zero and not read)
    const uint32_t nc = (!gate || *gate != 0) ? ncopy : 1;
    unsigned e = 0;
    for (uint32_t k = blockIdx.x * RSD_THREADS + threadIdx.x; k < K; k += gridDim.x * RSD_THREADS) {
        uint64_t n = sums[cnt0 + k];
        for (uint32_t i = 1; i < nc; i++) n += sums[i * cstride + cnt0 + k];
        w.cnt[k] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
        w.E[k] = 0;
        w.far[k] = 0;
        e += n == 0;
    }
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int i = 0; i < RSD_THREADS / 64; i++) t += wsum[i];
        if (t) atomicAdd(w.state, t);
    }
}

// A lane per row, grid-stride.  LDS: the block's E and far in shared memory (K <= RSD_LDS_K), one
// global add and max per cell the block met; else the lanes of a wave that share a cell are
// reduced first and one lane per cell and wave goes to global memory.
template <bool LDS>
__global__ __launch_bounds__(RSD_THREADS) void reseed_rows_kernel(const uint8_t *__restrict__ codes, uint32_t Dp,
                                                                  uint32_t D, uint64_t N,
                                                                  const uint32_t *__restrict__ A,
                                                                  const double *__restrict__ C, uint32_t K,
                                                                  const double *__restrict__ lut64, int shift,
                                                                  ReseedWork w) {
    if (*w.state == 0) return;   // no empty cell: nothing to seed (the same for every thread)
    __shared__ double lut[256];
    __shared__ ull sE[LDS ? RSD_LDS_K : 1], sF[LDS ? RSD_LDS_K : 1];
    static_assert(RSD_THREADS == 256, "one table entry per thread");
    lut[threadIdx.x] = lut64[threadIdx.x];
    if (LDS)
        for (uint32_t k = threadIdx.x; k < K; k += RSD_THREADS) sE[k] = sF[k] = 0;
    __syncthreads();
    ull *gE = reinterpret_cast<ull *>(w.E), *gF = reinterpret_cast<ull *>(w.far);
    const int lane = (int)(threadIdx.x & 63);
    for (uint64_t base = (uint64_t)blockIdx.x * RSD_THREADS; base < N; base += (uint64_t)gridDim.x * RSD_THREADS) {
        const uint64_t row = base + threadIdx.x;
        uint32_t k = 0, q = 0;
        bool active = row < N;
        if (active) {
            k = A[row];
            active = k < K;   // (never false: A is the search's)
        }
        if (active) {
            const uint32_t *xw = reinterpret_cast<const uint32_t *>(codes + row * Dp);
            const double *c = C + (uint64_t)k * D;
            double e = 0.0;
            if ((D & 1) == 0) {   // an even width: the code vector in 16-byte loads (half the gathers)
                const double2 *c2 = reinterpret_cast<const double2 *>(c);
                for (uint32_t i = 0; i < Dp / 4; i++) {
                    const uint32_t word = xw[i];
                    for (uint32_t b = 0; b < 4; b += 2) {
                        const uint32_t d = 4 * i + b;
                        if (d < D) {
                            const double2 cv = c2[d / 2];
                            e = reseed_error_step(e, lut[(word >> (8 * b)) & 255u], cv.x);
                            e = reseed_error_step(e, lut[(word >> (8 * b + 8)) & 255u], cv.y);
                        }
                    }
                }
            } else {
                for (uint32_t i = 0; i < Dp / 4; i++) {
                    const uint32_t word = xw[i];
                    for (uint32_t b = 0; b < 4; b++) {
                        const uint32_t d = 4 * i + b;
                        if (d < D) e = reseed_error_step(e, lut[(word >> (8 * b)) & 255u], c[d]);
                    }
                }
            }
            q = reseed_quantise(e, shift);
        }
        const ull key = reseed_far_key(q, (uint32_t)row);
        if (LDS) {
            if (active) {
                if (q) atomicAdd(&sE[k], (ull)q);
                atomicMax(&sF[k], key);
            }
        } else {
            ull pending = __ballot(active);
            while (pending) {   // (wave-uniform)
                const int leader = __ffsll(pending) - 1;
                const uint32_t k0 = __shfl(k, leader);
                const bool mine = active && k == k0;
                const ull m = __ballot(mine);
                ull sq = mine ? (ull)q : 0ull, mk = mine ? key : 0ull;
                if (__popcll(m) > 1)
                    for (int off = 32; off >= 1; off >>= 1) {
                        sq += __shfl_xor(sq, off);
                        const ull o = __shfl_xor(mk, off);
                        mk = o > mk ? o : mk;
                    }
                if (lane == leader) {
                    if (sq) atomicAdd(&gE[k0], sq);
                    atomicMax(&gF[k0], mk);
                }
                pending &= ~m;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < K; k += RSD_THREADS)
            if (sF[k]) {   // (a row's key is never 0: row < 2^32 - 1)
                if (sE[k]) atomicAdd(&gE[k], sE[k]);
                atomicMax(&gF[k], sF[k]);
            }
    }
}

// One block.  The lists (empties ascending; donors in cell order, then sorted under
// reseed_before by a bitonic network, in LDS where they fit), the seeds, the count.
__global__ __launch_bounds__(RSD_SEL_THREADS) void reseed_select_kernel(const uint8_t *__restrict__ codes, uint32_t Dp,
                                                                        uint32_t D, uint64_t N,
                                                                        const double *__restrict__ lut64, double *C,
                                                                        uint32_t K, ReseedWork w, uint64_t *pub) {
    constexpr uint32_t T = RSD_SEL_THREADS;
    const uint32_t tid = threadIdx.x;
    if (*w.state == 0) {   // (the same for every thread)
        if (tid == 0) *pub = 0;
        return;
    }
    __shared__ uint32_t scan[T];
    __shared__ ull sE[RSD_SEL_LDS];
    __shared__ uint32_t sK[RSD_SEL_LDS];
    ull *dE = reinterpret_cast<ull *>(w.dE);
    uint32_t ne = 0, nd = 0;   // the lists' lengths so far (every thread's)
    for (uint32_t base = 0; base < K; base += T) {
        const uint32_t k = base + tid;
        bool fe = false, fd = false;
        uint64_t E = 0;
        if (k < K) {
            const uint32_t n = w.cnt[k];
            E = w.E[k];
            fe = n == 0;
            fd = reseed_is_donor(n, E);
        }
        const uint32_t v = (fe ? 1u : 0u) | (fd ? 1u << 16 : 0u);   // two counts <= 1024 in one word
        scan[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < T; off <<= 1) {
            const uint32_t a = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += a;
            __syncthreads();
        }
        const uint32_t excl = scan[tid] - v, total = scan[T - 1];
        __syncthreads();
        if (fe) w.empties[ne + (excl & 0xFFFFu)] = k;
        if (fd) {
            dE[nd + (excl >> 16)] = E;
            w.dK[nd + (excl >> 16)] = k;
        }
        ne += total & 0xFFFFu;
        nd += total >> 16;
    }
    const uint32_t m = min(ne, nd);
    if (m) {
        uint32_t Pn = 1;
        while (Pn < nd) Pn <<= 1;   // <= the lists' capacity, K rounded up to a power of two
        for (uint32_t i = nd + tid; i < Pn; i += T) {   // padding: after every donor
            dE[i] = 0;
            w.dK[i] = 0xFFFFFFFFu;
        }
        __syncthreads();
        const bool lds = Pn <= RSD_SEL_LDS;
        ull *pe = lds ? sE : dE;
        uint32_t *pk = lds ? sK : w.dK;
        if (lds) {
            for (uint32_t i = tid; i < Pn; i += T) {
                sE[i] = dE[i];
                sK[i] = w.dK[i];
            }
            __syncthreads();
        }
        for (uint32_t k2 = 2; k2 <= Pn; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < Pn; i += T) {
                    const uint32_t l = i ^ j;
                    if (l > i) {
                        const ull ea = pe[i], eb = pe[l];
                        const uint32_t ka = pk[i], kb = pk[l];
                        const bool up = (i & k2) == 0;
                        if (up ? reseed_before(eb, kb, ea, ka) : reseed_before(ea, ka, eb, kb)) {
                            pe[i] = eb;
                            pk[i] = kb;
                            pe[l] = ea;
                            pk[l] = ka;
                        }
                    }
                }
                __syncthreads();
            }
        // the seeds: cell empties[j] takes the far row of donor j, as fp64 values from the table
        for (uint64_t i = tid; i < (uint64_t)m * D; i += T) {
            const uint32_t j = (uint32_t)(i / D), d = (uint32_t)(i % D);
            const uint32_t donor = pk[j], row = reseed_far_row(w.far[donor]);
            if (donor < K && row < N)   // (always: a donor has rows)
                C[(uint64_t)w.empties[j] * D + d] = lut64[codes[(uint64_t)row * Dp + d]];
        }
    }
    if (tid == 0) {
        *w.state = 0;
        *pub = m;
    }
}

inline uint32_t pow2_at_least(uint32_t K) {
    uint32_t p = 1;
    while (p < K) p <<= 1;
    return p;
}

}  // namespace

ReseedLayout reseed_layout(uint32_t K) {
    ReseedLayout l;
    const uint64_t P = pow2_at_least(K);
    uint64_t o = 16;   // state
    l.E = o, o += 8ull * K;
    l.far = o, o += 8ull * K;
    l.dE = o, o += 8 * P;
    l.cnt = o, o += 4ull * K;
    l.empties = o, o += 4ull * K;
    l.dK = o, o += 4 * P;
    l.total = o;
    return l;
}

ReseedWork reseed_work(uint8_t *base, uint32_t K) {
    const ReseedLayout l = reseed_layout(K);
    ReseedWork w;
    w.state = reinterpret_cast<unsigned *>(base);
    w.E = reinterpret_cast<uint64_t *>(base + l.E);
    w.far = reinterpret_cast<uint64_t *>(base + l.far);
    w.dE = reinterpret_cast<uint64_t *>(base + l.dE);
    w.cnt = reinterpret_cast<uint32_t *>(base + l.cnt);
    w.empties = reinterpret_cast<uint32_t *>(base + l.empties);
    w.dK = reinterpret_cast<uint32_t *>(base + l.dK);
    return w;
}

hipError_t launch_reseed_count(hipStream_t s, const uint64_t *sums, uint32_t K, uint32_t D, uint32_t ncopy,
                               uint64_t cstride, const unsigned *gate, const ReseedWork &w) {
    if (!sums || K == 0 || K > (1u << 20) || D == 0 || D > 64 || ncopy == 0 || !w.state) return hipErrorInvalidValue;
    const uint64_t cell_u64 = 2 * (uint64_t)K * D + K;
    if (cstride && cstride < cell_u64) return hipErrorInvalidValue;
    const uint32_t grid = std::min<uint32_t>((K + RSD_THREADS - 1) / RSD_THREADS, RSD_GRID_CAP);
    hipLaunchKernelGGL(reseed_count_kernel, dim3(grid), dim3(RSD_THREADS), 0, s, sums, K, D, ncopy,
                       cstride ? cstride : cell_u64, gate, w);
    return hipGetLastError();
}

hipError_t launch_reseed_rows(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N,
                              const uint32_t *A, const double *C, uint32_t K, const double *lut64, bool scaled,
                              const ReseedWork &w) {
    if (!codes || !A || !C || !lut64 || !w.state || N == 0 || N >= 0xFFFFFFFFull || K == 0 || K > (1u << 20) ||
        D == 0 || D > 64 || Dp < D || (Dp & 3))
        return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((N + RSD_THREADS - 1) / RSD_THREADS, RSD_GRID_CAP);
    const int shift = reseed_shift(scaled);
    if (K <= RSD_LDS_K)
        hipLaunchKernelGGL(reseed_rows_kernel<true>, dim3(grid), dim3(RSD_THREADS), 0, s, codes, Dp, D, N, A, C, K,
                           lut64, shift, w);
    else
        hipLaunchKernelGGL(reseed_rows_kernel<false>, dim3(grid), dim3(RSD_THREADS), 0, s, codes, Dp, D, N, A, C, K,
                           lut64, shift, w);
    return hipGetLastError();
}

hipError_t launch_reseed_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N,
                                const double *lut64, double *C, uint32_t K, const ReseedWork &w, uint64_t *pub) {
    if (!codes || !lut64 || !C || !w.state || !pub || N == 0 || K == 0 || K > (1u << 20) || D == 0 || D > 64 ||
        Dp < D)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(reseed_select_kernel, dim3(1), dim3(RSD_SEL_THREADS), 0, s, codes, Dp, D, N, lut64, C, K, w,
                       pub);
    return hipGetLastError();
}

}  // namespace qvq
