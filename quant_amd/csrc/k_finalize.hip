// k_finalize.hip -- the finalize: exact centroids from the reduced sums, the split or (qvq_refine,
// DESIGN.md 3.11) the same K, the next search's tables, tile order and host copy, the closed-form
// distortion term; the same tables from a given codebook (qvq_assign) or from its split
// (qvq_lbg_lloyd); the rows that changed between two assignments; the cells
// without a row.  One kernel in five forms (FinArgs, common.hpp).
//
// Sums layout as k_misc.hip: hi[d][k] (K*D) | lo[d][k] (K*D) | cnt[k] (K), u64; further copies
// cstride apart (the mean's MEAN_COPIES; kd_reduce_kernel's moves of tie rows), added mod 2^64.
#include <algorithm>

#include "common.hpp"
#include "mfma_util.hpp"
#include "prune_order.hpp"

namespace qvq {

namespace {

// The kernel's argument: the launch argument and what launch_finalize derives from it.
struct FinDev : FinArgs {
    double scale_t;         // 2^t
    float *qproj;           // with perm: the rows' projections for prune_order (behind tint's envelopes)
    uint64_t *zero_after;   // zero_sums: cleared by the last block once every block has read the sums
    uint32_t n_zero;
    bool dist;              // the distortion term is wanted (dist_out, or pub with sums)
};

// The reduced sums of component d of cell k over the first ncopy copies, and their centroid
// (centroid_value: an empty cell is the zero vector).
struct Cell {
    uint64_t hs, ls, cnt;
    double cv;
};
__device__ inline Cell read_cell(const FinDev &a, uint32_t k, uint32_t d, uint32_t ncopy) {
    const uint64_t KD = (uint64_t)a.K * a.D, c = (uint64_t)d * a.K + k;
    Cell s{a.sums[c], a.sums[KD + c], a.sums[2 * KD + k], 0.0};
    for (uint32_t i = 1; i < ncopy; i++) {
        const uint64_t *p = a.sums + i * a.cstride;
        s.hs += p[c];
        s.ls += p[KD + c];
        s.cnt += p[2 * KD + k];
    }
    s.cv = centroid_value(s.hs, s.ls, s.cnt, a.R, a.bias, a.scale);
    return s;
}

// One component's part of the distortion term 2 c.S - n ||c||^2 of a cell with code vector
// component c: S = the sum of the cell's values of the component, rounded once.
__device__ inline double cell_term(const FinDev &a, const Cell &s, double c) {
    const __int128 Sq = (__int128)a.R * (__int128)s.hs + (__int128)s.ls - (__int128)a.bias * (__int128)s.cnt;
    const double S = ldexp(i128_to_double(Sq), -a.scale);
    return 2.0 * c * S - (double)s.cnt * c * c;
}

// The search tables of row j from component value v in lane d of the row's L lanes (L >= LO; all
// L lanes call): code: code vector j -- C_next / host_cb (if given), C32, the MFMA row (common.hpp:
// hi / lo at their slots, the norm at 2 LO), E32 (D = 12) and its projection for prune_order;
// else a padding row that never wins.  The norm and the projection are butterfly sums over the
// row's lanes.
__device__ inline void write_tables(const FinDev &a, uint32_t j, uint32_t d, uint32_t L, double v, bool code) {
    const uint32_t D = a.D, Dp = a.Dp;
    const uint32_t RF = cb_row_f16(D, Dp), LO = cb_lo_off(D, Dp);
    _Float16 *row = a.rows + (uint64_t)j * RF;
    if (!code) {
        if (d < Dp) a.C32[(uint64_t)j * Dp + d] = 0.f;
        if (a.E32 && d < 16) a.E32[(uint64_t)j * 16 + d] = d == D ? 1e30f : 0.f;   // never wins
        for (uint32_t i = d; i < RF; i += L) row[i] = (_Float16)(i == 2 * LO || i == 2 * LO + 1 ? MF_PAD_SCORE : 0.f);
        return;
    }
    if (d < D) {
        if (a.C_next) a.C_next[(uint64_t)j * D + d] = v;
        if (a.host_cb) a.host_cb[(uint64_t)j * D + d] = v;
    }
    if (d < Dp) a.C32[(uint64_t)j * Dp + d] = (float)v;
    const double cp = d < D ? v - a.mu : 0.0;
    if (a.qproj) {   // the projection sum_d (c_d - mu) / sx (any order: prune_order widens it by 1)
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
    if (a.E32 && d < 16)   // L = 16 lanes for D = 12
        a.E32[(uint64_t)j * 16 + d] = d < D ? (float)c2 : (d == D ? (float)n : 0.f);
}

// Rows the kernel walks: the table rows with their padding, or the K cells.
__device__ __host__ inline uint32_t fin_rows(const FinArgs &a) {
    return a.children ? std::max(a.children * a.K, a.Kpad) : a.K;
}

// One (row j, component lane d) item; L lanes per row.  Row j < children K is a code vector:
// child j / K of cell j mod K (split: factor 1.2, then 0.8; same K: the centroid itself), or
// without sums the same child of row j mod K of C_src (qvq_lbg_lloyd's split of a codebook that
// holds seeds); the rows above are padding.  Without tables row j < K is cell j.
// Returns the item's distortion term.
__device__ inline double finalize_item(const FinDev &a, uint32_t j, uint32_t d, uint32_t L, uint32_t ncopy) {
    const uint32_t K = a.K, D = a.D;
    const uint32_t codes = a.children == 2 ? 2 * K : K, k = j < K ? j : j - K;
    double v = 0.0, term = 0.0;
    if (j < codes && d < D) {
        if (a.sums) {
            const Cell s = read_cell(a, k, d, ncopy);
            if (a.measure) {
                v = a.C_src[(uint64_t)j * D + d];
            } else {
                if (j < K) a.C_cent[(uint64_t)j * D + d] = s.cv;
                v = a.children == 2 ? s.cv * (j < K ? (double)(1 + 0.2) : (double)(1 - 0.2)) : s.cv;
            }
            if (a.dist && j < K && s.cnt) term = cell_term(a, s, a.measure ? v : s.cv);
            // split: behind the rows the K cells' row counts (the tie check: a cell of <= 2 rows has
            // the reference's bits, a Kahan sum of one or two values being the rounded exact sum)
            if (a.children == 2 && a.host_cb && j < K && d == 0)
                reinterpret_cast<uint32_t *>(a.host_cb + 2ull * K * D)[k] =
                    s.cnt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s.cnt;
        } else {
            v = a.C_src[(uint64_t)k * D + d];   // (same K: k = j)
            if (a.children == 2) v *= j < K ? (double)(1 + 0.2) : (double)(1 - 0.2);
        }
    }
    if (a.children && j < fin_rows(a)) write_tables(a, j, d, L, v, j < codes);
    return term;
}

// The end of a block: its distortion partial (tree order over the block's threads; only when a
// distortion is wanted: 8 barriers fewer elsewhere), the done count, and in the last block the
// distortion total (block order), the clearing of the sums' further copies, the next search's
// tile order, and what goes to the host: pub[0] = *changed, pub[1] = the total's bits, then the
// ready number.  open: the further copies were read (the gate, read by every thread at the
// kernel's start: the last block clears the counter behind it).
__device__ void finalize_block_done(const FinDev &a, double term, bool open) {
    __shared__ double red[256];
    __shared__ double parts[512];
    __shared__ bool last;
    // one block (small codebooks): no count and no agent fence, only the system fence before the
    // ready number (two fences of ~2-3.5 us each were most of a small level's finalize)
    const bool one = gridDim.x == 1;
    // mapped host memory was written: every wave's stores complete before the barrier, and thread
    // 0's system-scope fence below releases them with the block's count (MI355X guide's producer
    // pattern: one fence per block, not one per thread)
    const bool mapped = a.host_cb || a.ties.out || a.pub;
    if (a.dist) red[threadIdx.x] = term;
    if (mapped) __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (a.dist)
        for (int w = (int)blockDim.x / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        if (one) {
            last = true;
        } else {
            if (a.dist) a.dist_part[blockIdx.x] = red[0];
            if (mapped) __threadfence_system();
            else __threadfence();
            last = atomicAdd(a.done, 1u) == gridDim.x - 1;
        }
    }
    __syncthreads();
    if (!last) return;
    double total = 0.0;   // (thread 0's)
    if (one) {
        if (a.dist) total = red[0];
    } else {
        __threadfence();
        if (a.dist) {   // the block partials, loaded in parallel, then added in block order
            for (uint32_t b = threadIdx.x; b < gridDim.x; b += blockDim.x) parts[b] = __builtin_nontemporal_load(&a.dist_part[b]);
            __syncthreads();
            if (threadIdx.x == 0)
                for (uint32_t b = 0; b < gridDim.x; b++) total += parts[b];
        }
    }
    if (open)   // every block has read the sums
        for (uint32_t i = threadIdx.x; i < a.n_zero; i += blockDim.x) a.zero_after[i] = 0;
    if (a.perm) prune_order(a.qproj, a.children * a.K, a.Kpad, a.perm, a.tint);
    if (a.clear_cnt) __syncthreads();   // (every thread has read the gate before its counter goes)
    if (threadIdx.x == 0) {
        *a.done = 0;
        if (a.dist_out) a.dist_out[0] = total;
        if (a.pub) {
            a.pub[0] = a.changed64 ? *a.changed64 : (a.changed ? (uint64_t)*a.changed : 0);
            a.pub[1] = a.dist ? (uint64_t)__double_as_longlong(total) : 0;
        }
        if (a.changed) *a.changed = 0;
        if (a.changed64) *a.changed64 = 0;
        if (a.clear_cnt) a.clear_cnt[0] = a.clear_cnt[1] = 0;
        if (a.ready) {
            __threadfence_system();
            *reinterpret_cast<volatile uint64_t *>(a.ready) = a.seq;
        }
    }
}

// finalize (src/Quantizer.cpp:79-94 fixCodebook + :129-138 split) fused with the next search's
// tables.  Block = 256 / L rows x L component lanes (L = 16, 32 or 64 >= Dp), grid-stride over
// groups of 256 / L rows.  Each wave fences its mapped-host writes once, after its last row (a
// system fence writes back the L2: per row it cost ~25 ns x rows).
__global__ __launch_bounds__(256) void finalize_kernel(FinDev a, uint32_t L) {
    const uint32_t d = threadIdx.x % L, r = threadIdx.x / L;
    const uint32_t per = 256 / L, n = fin_rows(a);
    // the gate, once per thread: without ties copy 1 is all zero, neither read nor cleared
    const bool open = !a.gate || *a.gate != 0;
    const uint32_t ncopy = open ? a.ncopy : 1;
    double term = 0.0;
    for (uint32_t j0 = blockIdx.x * per; j0 < n; j0 += gridDim.x * per) term += finalize_item(a, j0 + r, d, L, ncopy);
    if (a.ties.out) {   // the tie rows, a thread per 4 bytes of a row record
        const TieExport &t = a.ties;
        const uint32_t nt = *t.cnt, m = min(nt, t.cap), words = 2 + a.Dp / 4;
        uint32_t *o = reinterpret_cast<uint32_t *>(t.out);
        if (blockIdx.x == 0 && threadIdx.x == 0) o[0] = nt;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)m * words;
             i += (uint64_t)gridDim.x * blockDim.x) {
            const uint32_t k = (uint32_t)(i / words), w = (uint32_t)(i % words), row = t.rows[k];
            if (row >= t.n_rows) {   // (never: the recheck lists rows)
                o[2 + i] = ~0u;
                continue;
            }
            o[2 + i] = w == 0 ? row
                              : (w == 1 ? t.A[row] : reinterpret_cast<const uint32_t *>(t.codes + (uint64_t)row * a.Dp)[w - 2]);
        }
    }
    if (a.done) finalize_block_done(a, term, open);
}

// Rows whose code vector differs between two assignments: 16-byte loads, a wave reduction, one
// atomic per workgroup.  8 bytes of HBM traffic per row and nothing else.  T: the total's type
// (unsigned: one rank's counter; unsigned long long: the slot behind the level's sums, which is
// all-reduced with them).
constexpr int CHG_THREADS = 256;
template <typename T>
__global__ __launch_bounds__(CHG_THREADS) void count_changed_kernel(const uint32_t *__restrict__ A,
                                                                    const uint32_t *__restrict__ B, uint64_t N,
                                                                    T *__restrict__ out) {
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
        if (t) atomicAdd(out, (T)t);
    }
}

constexpr uint32_t FIN_ONE_BLOCK_ROWS = 64;   // split rows: K <= 32

// The cells without a row under a level's reduced sums, read as the finalize reads them (its copies
// under its gate, so before the finalize that clears them): one block, the count to mapped host
// memory, which the host reads behind the ready number of a later finalize on the stream.
__global__ __launch_bounds__(CHG_THREADS) void count_empty_kernel(const uint64_t *__restrict__ sums, uint32_t K,
                                                                  uint32_t D, uint32_t ncopy, uint64_t cstride,
                                                                  const unsigned *__restrict__ gate,
                                                                  uint64_t *__restrict__ out) {
    __shared__ unsigned wsum[CHG_THREADS / 64];
    const uint64_t cnt0 = 2ull * K * D;
    const uint32_t nc = (!gate || *gate != 0) ? ncopy : 1;
    unsigned e = 0;
    for (uint32_t k = threadIdx.x; k < K; k += CHG_THREADS) {
        uint64_t n = sums[cnt0 + k];
        for (uint32_t i = 1; i < nc; i++) n += sums[i * cstride + cnt0 + k];
        e += n == 0;
    }
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < CHG_THREADS / 64; w++) t += wsum[w];
        *out = t;
        __threadfence_system();
    }
}

}  // namespace

hipError_t launch_finalize(hipStream_t s, const FinArgs &f) {
    const uint64_t cell_u64 = 2 * (uint64_t)f.K * f.D + f.K;
    if (f.D == 0 || f.D > 64 || f.K == 0 || f.children > 2 || f.ncopy == 0) return hipErrorInvalidValue;
    if (f.sums ? (f.measure ? !f.C_src : !f.C_cent) : !f.C_src) return hipErrorInvalidValue;
    if (f.measure && (!f.sums || f.children)) return hipErrorInvalidValue;
    if (f.children && (f.Kpad < f.K || !f.C32 || !f.rows || ((f.sums || f.children == 2) && !f.C_next)))
        return hipErrorInvalidValue;
    if (f.children == 2 && !f.sums && f.C_next == f.C_src) return hipErrorInvalidValue;   // (row k is read for row k + K)
    if (f.ties.out && (!f.done || !f.ready || !f.ties.rows || !f.ties.cnt || !f.ties.A || !f.ties.codes || (f.Dp & 3) ||
                       !f.ties.n_rows))
        return hipErrorInvalidValue;   // released with the ready flag
    if (f.zero_sums && (!f.done || !f.sums || f.zero_skip >= f.ncopy)) return hipErrorInvalidValue;   // the last block's
    if (f.cstride && f.cstride < cell_u64) return hipErrorInvalidValue;
    // what the last block publishes needs its counter, and the host a ready number to wait for
    if ((f.dist_out || f.ready || f.pub || f.changed || f.changed64 || f.clear_cnt) && !f.done)
        return hipErrorInvalidValue;
    if (f.changed && f.changed64) return hipErrorInvalidValue;
    if (f.pub && (!f.ready || !f.dist_part)) return hipErrorInvalidValue;
    FinDev a;
    static_cast<FinArgs &>(a) = f;
    if (!a.cstride) a.cstride = cell_u64;   // the copies follow each other
    a.scale_t = std::ldexp(1.0, f.t);
    if (f.D != MF_D) a.E32 = nullptr;
    a.qproj = nullptr;
    if (f.perm) {   // the last block orders the next search's code vectors
        if (!f.done || !f.children || !f.tint || f.children * f.K > PRUNE_MAXK || f.Kpad % 32 || f.Kpad > PRUNE_MAXK)
            return hipErrorInvalidValue;
        a.qproj = reinterpret_cast<float *>(f.tint + 2 * PRUNE_MAXT);   // (the envelopes' region is fixed)
    }
    a.zero_after = nullptr;
    a.n_zero = 0;
    if (f.zero_sums) {   // copies zero_skip .. ncopy - 1
        a.zero_after = const_cast<uint64_t *>(f.sums) + (uint64_t)f.zero_skip * a.cstride;
        a.n_zero = (uint32_t)((f.ncopy - f.zero_skip - 1) * a.cstride + cell_u64);
    }
    a.dist = f.dist_out || (f.pub && f.sums);
    // small codebooks in one block (the grid-stride loop takes several rows per thread), which
    // needs no cross-block count or fence (finalize_block_done); else <= the 512 partials
    const uint32_t L = f.D <= 16 ? 16 : (f.D <= 32 ? 32 : 64), n = fin_rows(f);
    const uint32_t grid = n <= FIN_ONE_BLOCK_ROWS ? 1u : std::min<uint32_t>((n + 256 / L - 1) / (256 / L), 512);
    if (a.dist && grid > 1 && !f.dist_part) return hipErrorInvalidValue;
    hipLaunchKernelGGL(finalize_kernel, dim3(grid), dim3(256), 0, s, a, L);
    return hipGetLastError();
}

hipError_t launch_count_empty(hipStream_t s, const uint64_t *sums, uint32_t K, uint32_t D, uint32_t ncopy,
                              uint64_t cstride, const unsigned *gate, uint64_t *out) {
    if (!sums || !out || K == 0 || D == 0 || ncopy == 0 || (ncopy > 1 && cstride < 2ull * K * D + K))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(count_empty_kernel, dim3(1), dim3(CHG_THREADS), 0, s, sums, K, D, ncopy, cstride, gate, out);
    return hipGetLastError();
}

namespace {
inline int changed_grid(int num_cu, uint64_t N) {
    const uint64_t want = (N / 4 + CHG_THREADS - 1) / CHG_THREADS / 4 + 1;   // ~4 loads in flight per thread
    return (int)std::min<uint64_t>(want, (uint64_t)std::max(num_cu, 1) * 8);
}
}  // namespace

hipError_t launch_count_changed(hipStream_t s, int num_cu, const uint32_t *A, const uint32_t *B, uint64_t N,
                                unsigned *out) {
    if (!A || !B || !out || N == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(count_changed_kernel<unsigned>, dim3(changed_grid(num_cu, N)), dim3(CHG_THREADS), 0, s, A, B, N,
                       out);
    return hipGetLastError();
}

hipError_t launch_count_changed64(hipStream_t s, int num_cu, const uint32_t *A, const uint32_t *B, uint64_t N,
                                  uint64_t *out) {
    if (!A || !B || !out || N == 0) return hipErrorInvalidValue;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the u64 slot");
    hipLaunchKernelGGL(count_changed_kernel<unsigned long long>, dim3(changed_grid(num_cu, N)), dim3(CHG_THREADS), 0,
                       s, A, B, N, reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

}  // namespace qvq
