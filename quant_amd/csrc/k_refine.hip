// k_refine.hip -- Lloyd refinement at fixed K (qvq_refine): the centroid step
// without the split, fused with the next search's tables; the count of rows that changed their
// code vector; the distortion of a codebook under an assignment that is not its own.
//
// Sums layout as k_misc.hip: hi[d][k] (K*D) | lo[d][k] (K*D) | cnt[k] (K), u64; a second copy
// cstride further on holds the kd-tree ties' moves (kd_reduce_kernel), added mod 2^64.
#include <algorithm>

#include "common.hpp"
#include "mfma_util.hpp"
#include "prune_order.hpp"

namespace qvq {

namespace {

struct RefArgs {
    const uint64_t *sums;    // the reduced sums of the iteration's assignment (null: no centroid step)
    const double *C_src;     // sums == null: the codebook to prepare; dist only: the codebook measured
    uint32_t K, Kpad, D, Dp;
    int64_t R, bias;
    int scale;
    uint64_t cstride;        // u64 from copy 0 of the sums to copy 1
    const unsigned *gate;    // non-null: copy 1 is added (and cleared) when *gate != 0 (the tie count)
    double *C_cent;          // the centroids [K][D]
    double *C_next;          // ... again, as the codebook of the next search
    double mu, sx, scale_t;
    float *C32;
    _Float16 *rows;
    float *E32;
    double *host_cb;         // mapped host memory: the codebook for the host's kd-tree build
    uint32_t *perm;          // the next search's tile order (prune_order), or null
    int32_t *tint;
    float *qproj;
    double *dist_part;       // per-block partials of sum_k (2 c_k.S_k - n_k ||c_k||^2)
    unsigned *done;          // block counter at 0, left at 0
    unsigned *changed;       // count_changed_kernel's total: published, then cleared
    unsigned *clear_cnt;     // the iteration's flag and tie counters (2), cleared for the next one
    uint64_t *pub;           // mapped host memory: [0] rows changed, [1] the distortion term's bits
    volatile uint64_t *ready;
    uint64_t seq;
};

__device__ inline uint64_t ref_sum(const RefArgs &a, uint64_t i, bool two) {
    uint64_t v = a.sums[i];
    if (two) v += a.sums[a.cstride + i];
    return v;
}

// S = sum of the cell's values of one component, rounded once (as finalize_item's distortion term)
__device__ inline double ref_cell_sum(const RefArgs &a, uint64_t hs, uint64_t ls, uint64_t cnt) {
    const __int128 Sq = (__int128)a.R * (__int128)hs + (__int128)ls - (__int128)a.bias * (__int128)cnt;
    return ldexp(i128_to_double(Sq), -a.scale);
}

// Search tables of row j (< K: code vector j with component value v in lane d; K .. Kpad - 1:
// padding that never wins), the arithmetic of finalize_split_item / prep_row.
__device__ inline void ref_table_item(const RefArgs &a, uint32_t j, uint32_t d, uint32_t L, double v) {
    const uint32_t K = a.K, D = a.D, Dp = a.Dp;
    const uint32_t RF = cb_row_f16(D, Dp), LO = cb_lo_off(D, Dp);
    _Float16 *row = a.rows + (uint64_t)j * RF;
    if (j >= K) {
        if (d < Dp) a.C32[(uint64_t)j * Dp + d] = 0.f;
        if (a.E32 && d < 16) a.E32[(uint64_t)j * 16 + d] = d == D ? 1e30f : 0.f;
        for (uint32_t i = d; i < RF; i += L) row[i] = (_Float16)(i == 2 * LO || i == 2 * LO + 1 ? MF_PAD_SCORE : 0.f);
        return;
    }
    if (d < D) {
        a.C_next[(uint64_t)j * D + d] = v;
        if (a.host_cb) a.host_cb[(uint64_t)j * D + d] = v;
    }
    if (d < Dp) a.C32[(uint64_t)j * Dp + d] = (float)v;
    const double cp = d < D ? v - a.mu : 0.0;
    if (a.qproj) {
        double qs = cp;
        for (uint32_t off = L / 2; off >= 1; off >>= 1) qs += __shfl_xor(qs, (int)off, (int)L);
        if (d == 0) a.qproj[j] = (float)(qs / a.sx);
    }
    double n = cp * cp;
    for (uint32_t off = L / 2; off >= 1; off >>= 1) n += __shfl_xor(n, (int)off, (int)L);
    const double c2 = -2.0 * a.sx * cp * a.scale_t;
    if (d < D) {
        const _Float16 h = (_Float16)(float)c2;
        row[cb_hi_slot(D, Dp, d)] = h;
        row[cb_lo_slot(D, Dp, d)] = (_Float16)(float)(c2 - (double)(float)h);
    } else if (d < LO) {
        row[cb_hi_slot(D, Dp, d)] = (_Float16)0.f;
        row[cb_lo_slot(D, Dp, d)] = (_Float16)0.f;
    }
    n *= a.scale_t;
    const _Float16 h = (_Float16)(float)n;
    const _Float16 l = (_Float16)(float)(n - (double)(float)h);
    for (uint32_t i = 2 * LO + d; i < RF; i += L) row[i] = i == 2 * LO ? h : (i == 2 * LO + 1 ? l : (_Float16)0.f);
    if (a.E32 && d < 16) a.E32[(uint64_t)j * 16 + d] = d < D ? (float)c2 : (d == D ? (float)n : 0.f);
}

// The end of a block (the pattern of k_misc.hip's finalize_block_done): the block's distortion
// partial in tree order, the done count; the last block adds the partials in block order, clears
// copy 1 of the sums and the iteration's counters, orders the next search's tiles and publishes
// the changed count, the distortion term and the ready number to the host.
__device__ void refine_block_done(const RefArgs &a, double term, bool two) {
    __shared__ double red[256];
    __shared__ double parts[512];
    __shared__ bool last;
    const bool one = gridDim.x == 1;
    red[threadIdx.x] = term;
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the mapped stores, before the barrier
    __syncthreads();
    for (int w = (int)blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (one) {
            last = true;
        } else {
            a.dist_part[blockIdx.x] = red[0];
            __threadfence_system();
            last = atomicAdd(a.done, 1u) == gridDim.x - 1;
        }
    }
    __syncthreads();
    if (!last) return;
    if (!one) {
        __threadfence();
        for (uint32_t b = threadIdx.x; b < gridDim.x; b += blockDim.x) parts[b] = __builtin_nontemporal_load(&a.dist_part[b]);
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0;
            for (uint32_t b = 0; b < gridDim.x; b++) t += parts[b];
            red[0] = t;
        }
    }
    if (two) {   // every block has read the sums: copy 1 back to zero for the next kd_reduce
        const uint64_t n = 2 * (uint64_t)a.K * a.D + a.K;
        uint64_t *s1 = const_cast<uint64_t *>(a.sums) + a.cstride;
        for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) s1[i] = 0;
    }
    if (a.perm) prune_order(a.qproj, a.K, a.Kpad, a.perm, a.tint);
    __syncthreads();   // (two was read from *gate by every thread before the counters go)
    if (threadIdx.x == 0) {
        *a.done = 0;
        a.pub[0] = a.changed ? (uint64_t)*a.changed : 0;
        a.pub[1] = (uint64_t)__double_as_longlong(red[0]);
        if (a.changed) *a.changed = 0;
        if (a.clear_cnt) a.clear_cnt[0] = a.clear_cnt[1] = 0;
        __threadfence_system();
        *a.ready = a.seq;
    }
}

// The centroid step of one refinement iteration, in place of finalize_prep_kernel: row j < K is
// the exact centroid of cell j (centroid_value: the rounding of launch_finalize and
// qvq_host_finalize; an empty cell is the zero vector), written as the iteration's codebook and
// as the next search's, with that search's tables for the same K; no split.  sums == null: the
// tables of the codebook C_src (the refinement's starting point).  Block = 256 / L rows x L
// component lanes (L = 16, 32 or 64 >= Dp), grid-stride.
__global__ __launch_bounds__(256) void refine_finalize_kernel(RefArgs a, uint32_t L) {
    const uint32_t d = threadIdx.x % L, r = threadIdx.x / L, per = 256 / L;
    const uint32_t K = a.K, D = a.D;
    const uint64_t KD = (uint64_t)K * D;
    const bool two = a.sums && a.gate && *a.gate != 0;
    double term = 0.0;
    for (uint32_t j0 = blockIdx.x * per; j0 < a.Kpad; j0 += gridDim.x * per) {
        const uint32_t j = j0 + r;
        double v = 0.0;
        if (j < K && d < D) {
            if (a.sums) {
                const uint64_t c = (uint64_t)d * K + j;
                const uint64_t cnt = ref_sum(a, 2 * KD + j, two), hs = ref_sum(a, c, two), ls = ref_sum(a, KD + c, two);
                v = centroid_value(hs, ls, cnt, a.R, a.bias, a.scale);
                a.C_cent[(uint64_t)j * D + d] = v;
                if (cnt) term += 2.0 * v * ref_cell_sum(a, hs, ls, cnt) - (double)cnt * v * v;
            } else {
                v = a.C_src[(uint64_t)j * D + d];
            }
        }
        if (j < a.Kpad) ref_table_item(a, j, d, L, v);
    }
    refine_block_done(a, term, two);
}

// sum_k (2 c_k.S_k - n_k ||c_k||^2) for the codebook C_src and the sums of an assignment that need
// not be its own (QVQ_REFINE_FRESH): with sum ||x||^2 the distortion in closed form.  Same
// blocks and publication as refine_finalize_kernel; writes no codebook and no tables.
__global__ __launch_bounds__(256) void refine_dist_kernel(RefArgs a, uint32_t L) {
    const uint32_t d = threadIdx.x % L, r = threadIdx.x / L, per = 256 / L;
    const uint32_t K = a.K, D = a.D;
    const uint64_t KD = (uint64_t)K * D;
    const bool two = a.gate && *a.gate != 0;
    double term = 0.0;
    for (uint32_t j0 = blockIdx.x * per; j0 < K; j0 += gridDim.x * per) {
        const uint32_t j = j0 + r;
        if (j < K && d < D) {
            const uint64_t c = (uint64_t)d * K + j;
            const uint64_t cnt = ref_sum(a, 2 * KD + j, two), hs = ref_sum(a, c, two), ls = ref_sum(a, KD + c, two);
            const double v = a.C_src[(uint64_t)j * D + d];
            if (cnt) term += 2.0 * v * ref_cell_sum(a, hs, ls, cnt) - (double)cnt * v * v;
        }
    }
    refine_block_done(a, term, two);
}

// Rows whose code vector differs between two assignments: 16-byte loads, a wave reduction, one
// atomic per workgroup.  8 bytes of HBM traffic per row and nothing else.
constexpr int CHG_THREADS = 256;
__global__ __launch_bounds__(CHG_THREADS) void count_changed_kernel(const uint32_t *__restrict__ A,
                                                                    const uint32_t *__restrict__ B, uint64_t N,
                                                                    unsigned *__restrict__ out) {
    __shared__ unsigned wsum[CHG_THREADS / 64];
    const uint64_t n4 = N / 4;
    const uint4 *A4 = reinterpret_cast<const uint4 *>(A), *B4 = reinterpret_cast<const uint4 *>(B);
    unsigned c = 0;
    const uint64_t tid = (uint64_t)blockIdx.x * CHG_THREADS + threadIdx.x, step = (uint64_t)gridDim.x * CHG_THREADS;
    for (uint64_t i = tid; i < n4; i += step) {
        const uint4 x = A4[i], y = B4[i];
        c += (x.x != y.x) + (x.y != y.y) + (x.z != y.z) + (x.w != y.w);
    }
    for (uint64_t i = 4 * n4 + tid; i < N; i += step) c += A[i] != B[i];
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < CHG_THREADS / 64; w++) t += wsum[w];
        if (t) atomicAdd(out, t);
    }
}

uint32_t ref_lanes(uint32_t D) { return D <= 16 ? 16 : (D <= 32 ? 32 : 64); }
uint32_t ref_grid(uint32_t rows, uint32_t L) {   // <= the 512 partials of refine_block_done
    return rows <= 64 ? 1u : std::min<uint32_t>((rows + 256 / L - 1) / (256 / L), 512);
}

}  // namespace

hipError_t launch_refine_finalize(hipStream_t s, const RefineArgs &r) {
    if (r.D == 0 || r.D > 64 || r.K == 0 || r.Kpad < r.K || !r.done || !r.pub || !r.ready || !r.dist_part)
        return hipErrorInvalidValue;
    if (!r.sums && !r.C_src) return hipErrorInvalidValue;
    if (r.sums && r.gate && r.cstride < 2 * (uint64_t)r.K * r.D + r.K) return hipErrorInvalidValue;
    if (r.perm && (r.K > PRUNE_MAXK || r.Kpad % 32 || r.Kpad > PRUNE_MAXK || !r.tint)) return hipErrorInvalidValue;
    RefArgs a;
    a.sums = r.sums;
    a.C_src = r.C_src;
    a.K = r.K;
    a.Kpad = r.Kpad;
    a.D = r.D;
    a.Dp = r.Dp;
    a.R = r.R;
    a.bias = r.bias;
    a.scale = r.scale;
    a.cstride = r.cstride;
    a.gate = r.gate;
    a.C_cent = r.C_cent;
    a.C_next = r.C_next;
    a.mu = r.mu;
    a.sx = r.sx;
    a.scale_t = std::ldexp(1.0, r.t);
    a.C32 = r.C32;
    a.rows = r.rows;
    a.E32 = r.D == MF_D ? r.E32 : nullptr;
    a.host_cb = r.host_cb;
    a.perm = r.perm;
    a.tint = r.tint;
    a.qproj = r.perm ? reinterpret_cast<float *>(r.tint + 2 * PRUNE_MAXT) : nullptr;
    a.dist_part = r.dist_part;
    a.done = r.done;
    a.changed = r.changed;
    a.clear_cnt = r.clear_cnt;
    a.pub = r.pub;
    a.ready = r.ready;
    a.seq = r.seq;
    const uint32_t L = ref_lanes(r.D);
    if (r.tables) {
        if (!r.C_next || !r.C32 || !r.rows || (r.sums && !r.C_cent)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(refine_finalize_kernel, dim3(ref_grid(r.Kpad, L)), dim3(256), 0, s, a, L);
    } else {
        if (!r.sums || !r.C_src) return hipErrorInvalidValue;
        a.perm = nullptr;
        hipLaunchKernelGGL(refine_dist_kernel, dim3(ref_grid(r.K, L)), dim3(256), 0, s, a, L);
    }
    return hipGetLastError();
}

hipError_t launch_count_changed(hipStream_t s, int num_cu, const uint32_t *A, const uint32_t *B, uint64_t N,
                                unsigned *out) {
    if (!A || !B || !out || N == 0) return hipErrorInvalidValue;
    const uint64_t want = (N / 4 + CHG_THREADS - 1) / CHG_THREADS / 4 + 1;   // ~4 loads in flight per thread
    const int grid = (int)std::min<uint64_t>(want, (uint64_t)std::max(num_cu, 1) * 8);
    hipLaunchKernelGGL(count_changed_kernel, dim3(grid), dim3(CHG_THREADS), 0, s, A, B, N, out);
    return hipGetLastError();
}

}  // namespace qvq
