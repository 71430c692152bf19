// k_mediancut.hip -- qvq_median_cut's levels (the rule in median_cut_rule.hpp, the
// dispatch in median_cut_plan.hpp).  Level l, half = 2^(l-1) boxes, is four launches:
//   rows:  a lane per row: the row's label under level l - 1's cuts (written back), and the ranges
//          lo[b][d], hi[b][d] of its ordinals into the label's box (privatised in LDS, in groups of
//          boxes where one block's LDS does not hold them all);
//   axis:  a lane per box: the cut axis from the ranges, sel[b] = (axis, lo, hi, pending | none);
//          the level's histograms cleared;
//   hist:  a lane per row: h[b][u] += 1 on the axis of the row's box (boxes that are not cut skipped);
//   cut:   a block per box: t from the histogram (a scan and a key minimum), sel[b].t, the level's cut count; the ranges of the
//          box's two children reset for level l + 1.
// One more rows launch without ranges applies the last level's cuts.  Everything is integer minima,
// maxima and adds: the results do not depend on the order of the atomics.
#include <algorithm>

#include "common.hpp"
#include "median_cut_plan.hpp"
#include "median_cut_rule.hpp"

namespace qvq {

namespace {

constexpr uint32_t MC_NONE = 0xFFFFFFFFu;      // sel[b].t: the box is not cut
constexpr uint32_t MC_PENDING = 0xFFFFFFFEu;   // ... is cut, t not chosen yet (between axis and cut)

// lo and hi only ever fall and rise: a value read earlier bounds the current one, so a row inside
// the range read needs no atomic (after a box's first rows almost none does).
__device__ inline void mc_widen(uint32_t *lo, uint32_t *hi, uint32_t u) {
    if (u < __atomic_load_n(lo, __ATOMIC_RELAXED)) atomicMin(lo, u);
    if (u > __atomic_load_n(hi, __ATOMIC_RELAXED)) atomicMax(hi, u);
}

// half_prev = 0: level 1, every row in box 0.  Else the labels in A are below half_prev and sel
// holds the previous level's cuts.  ACC: the ranges of the nb = max(1, 2 half_prev) boxes.  LDS:
// blockIdx.y is a group of gp = gboxes / 2 parents (level 1: the one box) whose gboxes children
// sit in the block's LDS; the block reads every row's label and takes its parents' rows only, then
// sends one global min and max per entry it met.  Else (one group, gboxes = nb) the rows go
// straight to global memory.
template <bool LDS, bool ACC>
__global__ __launch_bounds__(MC_THREADS) void mc_rows_kernel(const uint8_t *__restrict__ codes, uint32_t Dp, uint32_t D,
                                                             uint64_t N, uint32_t *__restrict__ A,
                                                             const uint4 *__restrict__ sel, uint32_t half_prev,
                                                             uint32_t gboxes, uint32_t *glo, uint32_t *ghi) {
    __shared__ uint32_t sm[LDS && ACC ? MC_LDS_WORDS : 1];
    const uint32_t words = gboxes * D;   // LDS: lo [words] | hi [words]
    const uint32_t gp = gboxes / 2, p0 = blockIdx.y * gp;   // the group's parents p0 .. p0 + gp - 1
    if (LDS && ACC) {
        for (uint32_t i = threadIdx.x; i < words; i += MC_THREADS) sm[i] = 0xFFFFFFFFu, sm[words + i] = 0;
        __syncthreads();
    }
    for (uint64_t base = (uint64_t)blockIdx.x * MC_THREADS; base < N; base += (uint64_t)gridDim.x * MC_THREADS) {
        const uint64_t row = base + threadIdx.x;
        if (row >= N) continue;
        const uint8_t *x = codes + row * Dp;
        uint32_t b = 0, local = 0;
        if (half_prev) {
            b = A[row];
            if (b >= half_prev) continue;   // (never: the labels are this call's own)
            if (LDS && ACC && (b < p0 || b - p0 >= gp)) continue;   // another group's row
            local = b - p0;
            const uint4 s = sel[b];
            if (s.w <= 255u) {
                const uint32_t child = mc_relabel(b, mc_ordinal(x[s.x]), s.w, half_prev);
                if (child != b) local += gp;   // the upper children follow the group's lower ones
                b = child;
            }
        }
        A[row] = b;
        if (!ACC) continue;
        uint32_t *lo = LDS ? sm + local * D : glo + (uint64_t)b * D;
        uint32_t *hi = LDS ? sm + words + local * D : ghi + (uint64_t)b * D;
        auto word = [&](uint32_t w, uint32_t d0) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (d0 + j < D) mc_widen(lo + d0 + j, hi + d0 + j, mc_ordinal(w >> (8 * j)));
        };
        if ((Dp & 15) == 0) {   // rows of whole 16-byte pieces
            const uint4 *x4 = reinterpret_cast<const uint4 *>(x);
            for (uint32_t i = 0; i < Dp / 16; i++) {
                const uint4 v = x4[i];
                word(v.x, 16 * i), word(v.y, 16 * i + 4), word(v.z, 16 * i + 8), word(v.w, 16 * i + 12);
            }
        } else {
            const uint32_t *x1 = reinterpret_cast<const uint32_t *>(x);
            for (uint32_t i = 0; i < Dp / 4; i++) word(x1[i], 4 * i);
        }
    }
    if (LDS && ACC) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < words; i += MC_THREADS)
            if (sm[i] != 0xFFFFFFFFu) {   // the block met the entry's box
                const uint32_t l = i / D, d = i - l * D;
                const uint64_t g = (uint64_t)(l < gp || !half_prev ? p0 + l : half_prev + p0 + (l - gp)) * D + d;
                if (sm[i] < __atomic_load_n(glo + g, __ATOMIC_RELAXED)) atomicMin(glo + g, sm[i]);
                if (sm[words + i] > __atomic_load_n(ghi + g, __ATOMIC_RELAXED)) atomicMax(ghi + g, sm[words + i]);
            }
    }
}

// A lane per histogram word clears it; the first `boxes` lanes choose their box's axis.
__global__ __launch_bounds__(MC_THREADS) void mc_axis_kernel(const uint32_t *__restrict__ glo,
                                                             const uint32_t *__restrict__ ghi, uint32_t boxes, uint32_t D,
                                                             uint4 *__restrict__ sel, uint32_t *__restrict__ hist) {
    const uint64_t i = (uint64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i < 256ull * boxes) hist[i] = 0;
    if (i < boxes) {
        uint32_t range;
        const uint32_t axis = mc_axis(glo + i * D, ghi + i * D, D, &range);
        uint4 s;
        s.x = axis;
        s.y = range ? glo[i * D + axis] : 0;
        s.z = range ? ghi[i * D + axis] : 0;
        s.w = range ? MC_PENDING : MC_NONE;
        sel[i] = s;
    }
}

// LDS: blockIdx.y is a group of gboxes boxes whose bins sit in the block's LDS; the block reads every
// row's label and counts its boxes' rows only.  Else one group, global adds.
template <bool LDS>
__global__ __launch_bounds__(MC_THREADS) void mc_hist_kernel(const uint8_t *__restrict__ codes, uint32_t Dp, uint64_t N,
                                                             const uint32_t *__restrict__ A,
                                                             const uint4 *__restrict__ sel, uint32_t boxes,
                                                             uint32_t gboxes, uint32_t *ghist) {
    __shared__ uint32_t sm[LDS ? MC_LDS_WORDS : 1];
    const uint32_t words = 256 * gboxes, b0 = blockIdx.y * gboxes;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < words; i += MC_THREADS) sm[i] = 0;
        __syncthreads();
    }
    for (uint64_t base = (uint64_t)blockIdx.x * MC_THREADS; base < N; base += (uint64_t)gridDim.x * MC_THREADS) {
        const uint64_t row = base + threadIdx.x;
        if (row >= N) continue;
        const uint32_t b = A[row];
        if (b >= boxes) continue;   // (never)
        if (LDS && (b < b0 || b - b0 >= gboxes)) continue;   // another group's row
        const uint4 s = sel[b];
        if (s.w == MC_NONE) continue;
        const uint32_t u = mc_ordinal(codes[row * Dp + s.x]);
        if (LDS) atomicAdd(&sm[256 * (b - b0) + u], 1u);
        else atomicAdd(&ghist[256ull * b + u], 1u);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < words; i += MC_THREADS)
            if (sm[i]) atomicAdd(&ghist[256ull * b0 + i], sm[i]);
    }
}

// A block per box.  The two children's ranges are reset whether the box is cut or not: box b's
// own entries are read for the last time by the axis launch before.
__global__ __launch_bounds__(MC_THREADS) void mc_cut_kernel(const uint32_t *__restrict__ hist, uint32_t boxes, uint32_t D,
                                                            uint4 *__restrict__ sel, uint32_t *__restrict__ glo,
                                                            uint32_t *__restrict__ ghi, uint32_t *__restrict__ cuts) {
    static_assert(MC_THREADS == 256, "one bin per thread");
    __shared__ unsigned long long wsum[MC_THREADS / 64];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (tid < D) {
        glo[(uint64_t)b * D + tid] = 0xFFFFFFFFu, ghi[(uint64_t)b * D + tid] = 0;
        glo[((uint64_t)b + boxes) * D + tid] = 0xFFFFFFFFu, ghi[((uint64_t)b + boxes) * D + tid] = 0;
    }
    const uint4 s = sel[b];
    if (s.w == MC_NONE) return;   // (the same for every thread)
    // cum(v) by an inclusive scan over the 256 bins (a bin per thread: within the wave, then over
    // the four waves' totals), then the minimum of mc_cut_key over v in [lo, hi - 1]
    const uint32_t lane = tid & 63, wv = tid >> 6;
    unsigned long long cum = hist[256ull * b + tid];
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(cum, off);
        if ((int)lane >= off) cum += o;
    }
    if (lane == 63) wsum[wv] = cum;
    __syncthreads();
    unsigned long long n = 0;
    for (uint32_t i = 0; i < MC_THREADS / 64; i++) {
        if (i < wv) cum += wsum[i];
        n += wsum[i];
    }
    unsigned long long key = tid >= s.y && tid < s.z ? mc_cut_key(mc_balance(cum, n), tid) : ~0ull;
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    __syncthreads();   // (the totals are read: the slots take the waves' minima)
    if (lane == 0) wsum[wv] = key;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t i = 1; i < MC_THREADS / 64; i++) key = wsum[i] < key ? wsum[i] : key;
        sel[b].w = (uint32_t)(key & 255u);
        atomicAdd(cuts, 1u);
    }
}

// Level 1's box: its ranges reset, the call's cut counts cleared.
__global__ void mc_init_kernel(uint32_t D, uint32_t *__restrict__ glo, uint32_t *__restrict__ ghi,
                               uint32_t *__restrict__ cuts) {
    const uint32_t tid = threadIdx.x;
    if (tid < D) glo[tid] = 0xFFFFFFFFu, ghi[tid] = 0;
    if (tid < 32) cuts[tid] = 0;
}

}  // namespace

McLayout mc_layout(uint32_t K, uint32_t D) {
    const uint64_t boxes = std::max<uint32_t>(K / 2, 1);   // the last level's boxes
    McLayout l;
    uint64_t o = 0;
    l.cuts = o, o += 32 * 4;
    l.sel = o, o += 16 * boxes;
    l.lo = o, o += 4 * 2 * boxes * D;   // (the last cut resets its boxes' children)
    l.hi = o, o += 4 * 2 * boxes * D;
    l.hist = o, o += 4 * 256 * boxes;
    l.total = o;
    return l;
}

McWork mc_work(uint8_t *base, uint32_t K, uint32_t D) {
    const McLayout l = mc_layout(K, D);
    McWork w;
    w.cuts = reinterpret_cast<uint32_t *>(base + l.cuts);
    w.sel = reinterpret_cast<uint4 *>(base + l.sel);
    w.lo = reinterpret_cast<uint32_t *>(base + l.lo);
    w.hi = reinterpret_cast<uint32_t *>(base + l.hi);
    w.hist = reinterpret_cast<uint32_t *>(base + l.hist);
    return w;
}

hipError_t launch_mc_init(hipStream_t s, uint32_t D, const McWork &w) {
    if (!w.cuts || D == 0 || D > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mc_init_kernel, dim3(1), dim3(64), 0, s, D, w.lo, w.hi, w.cuts);
    return hipGetLastError();
}

hipError_t launch_mc_rows(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N, uint32_t *A,
                          uint32_t half_prev, bool ranges, const McWork &w) {
    if (!codes || !A || !w.cuts || N == 0 || D == 0 || D > 64 || Dp < D || (Dp & 3) || half_prev > (1u << 19) ||
        (half_prev & (half_prev - 1)))
        return hipErrorInvalidValue;
    const uint32_t nb = std::max<uint32_t>(1, 2 * half_prev);
    const MedianCutPlan p = median_cut_plan(D, nb, N);
    const dim3 block(MC_THREADS);
    if (!ranges)
        hipLaunchKernelGGL((mc_rows_kernel<false, false>), dim3(mc_grid(N, MC_GRID_CAP)), block, 0, s, codes, Dp, D, N, A,
                           w.sel, half_prev, nb, w.lo, w.hi);
    else if (p.range_lds)
        hipLaunchKernelGGL((mc_rows_kernel<true, true>), dim3(p.range_grid, p.range_groups), block, 0, s, codes, Dp, D, N,
                           A, w.sel, half_prev, p.range_group_boxes, w.lo, w.hi);
    else
        hipLaunchKernelGGL((mc_rows_kernel<false, true>), dim3(p.range_grid), block, 0, s, codes, Dp, D, N, A, w.sel,
                           half_prev, nb, w.lo, w.hi);
    return hipGetLastError();
}

hipError_t launch_mc_axis(hipStream_t s, uint32_t boxes, uint32_t D, const McWork &w) {
    if (!w.cuts || boxes == 0 || boxes > (1u << 19) || D == 0 || D > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mc_axis_kernel, dim3(boxes), dim3(MC_THREADS), 0, s, w.lo, w.hi, boxes, D, w.sel, w.hist);
    return hipGetLastError();
}

hipError_t launch_mc_hist(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N, const uint32_t *A,
                          uint32_t boxes, const McWork &w) {
    if (!codes || !A || !w.cuts || N == 0 || boxes == 0 || boxes > (1u << 19) || D == 0 || D > 64 || Dp < D)
        return hipErrorInvalidValue;
    const MedianCutPlan p = median_cut_plan(D, boxes, N);
    if (p.hist_lds)
        hipLaunchKernelGGL(mc_hist_kernel<true>, dim3(p.hist_grid, p.hist_groups), dim3(MC_THREADS), 0, s, codes, Dp, N, A,
                           w.sel, boxes, p.hist_group_boxes, w.hist);
    else
        hipLaunchKernelGGL(mc_hist_kernel<false>, dim3(p.hist_grid), dim3(MC_THREADS), 0, s, codes, Dp, N, A, w.sel, boxes,
                           boxes, w.hist);
    return hipGetLastError();
}

hipError_t launch_mc_cut(hipStream_t s, uint32_t boxes, uint32_t D, uint32_t level, const McWork &w) {
    if (!w.cuts || boxes == 0 || boxes > (1u << 19) || D == 0 || D > 64 || level == 0 || level > 20)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mc_cut_kernel, dim3(boxes), dim3(MC_THREADS), 0, s, w.hist, boxes, D, w.sel, w.lo, w.hi,
                       w.cuts + (level - 1));
    return hipGetLastError();
}

}  // namespace qvq
