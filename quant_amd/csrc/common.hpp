// common.hpp -- shared numerics and kernel launch interface of the qvq engine.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kdtree_dev.hpp"

namespace qvq {

// ---------------------------------------------------------------------------------------
// Exact-sum decomposition of a colour space's byte -> value map.
// Every value v[b] is an integer multiple of 2^-scale: q[b] = v[b] * 2^scale.  We write
// q[b] = R * hi[b] + (lo[b] - bias) with hi[b] <= 255 and 0 <= lo[b] <= 2*bias small, so one
// u64 LDS atomic of (hi << 32 | lo) per component accumulates both parts without carries
// for up to 2^24 rows per workgroup; the finaliser rebuilds the exact 128-bit sum.
//
// For the MFMA search every value is also an exact small integer in centred form:
// v[b] - mu = w[b] * sx with |w[b]| <= 255 (f16-exact), up to fl() rounding of v.
// ---------------------------------------------------------------------------------------
struct Terms {
    double v64[256];
    float v32[256];
    uint32_t hi[256];
    uint32_t lo[256];
    float w[256];       // centred integer value of each byte
    int64_t R;
    int64_t bias;
    int scale;
    uint8_t pad_code;   // byte whose value is exactly 0.0 (padding past the raster end)
    double vmax;        // max |v|
    double mu, sx;      // v ~= mu + w * sx
};

bool make_terms(int cs, Terms &t);

// Correctly rounded (nearest-even) conversion of a signed 128-bit integer to double.
__host__ __device__ inline double i128_to_double(__int128 v) {
    const bool neg = v < 0;
    unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
    if (hi == 0 && (lo >> 53) == 0) {
        const double d = (double)lo;   // exact
        return neg ? -d : d;
    }
#ifdef __HIP_DEVICE_COMPILE__
    const int lz = hi ? __clzll((long long)hi) : 64 + __clzll((long long)lo);
#else
    const int lz = hi ? __builtin_clzll(hi) : 64 + __builtin_clzll(lo);
#endif
    const int sh = (128 - lz) - 53;
    uint64_t top = (uint64_t)(m >> sh);
    const unsigned __int128 rem = m & (((unsigned __int128)1 << sh) - 1);
    const unsigned __int128 half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (top & 1))) top++;
    const double d = ldexp((double)top, sh);
    return neg ? -d : d;
}

// Centroid component from reduced sums: round(R*hi + lo - bias*cnt) * 2^-scale * fl(1/cnt).
// Empty cell -> zero vector (src/Quantizer.cpp:81-85).  The reciprocal multiply is the
// reference's operator/= under -freciprocal-math (include/VectorOperations.hpp:96-98).
__host__ __device__ inline double centroid_value(uint64_t hi, uint64_t lo, uint64_t cnt, int64_t R, int64_t bias,
                                                 int scale) {
    if (cnt == 0) return 0.0;
    const __int128 S = (__int128)R * (__int128)hi + (__int128)lo - (__int128)bias * (__int128)cnt;
    return ldexp(i128_to_double(S), -scale) * (1.0 / (double)cnt);
}

// MFMA search layout (D = 12): per code vector one 56-byte row of 28 f16
// [hi0..3, lo0..3, hi4..7, lo4..7, hi8..11, lo8..11, nhi, nlo, 0, 0], where hi+lo ~=
// -2*sx*(c-mu)*2^t and nhi+nlo ~= 2^t*||c-mu||^2, so that score = 2^t*(||x-c||^2 - ||x-mu||^2).
// K-slot group g < 3 (slots 8g..8g+7) then meets components 4g..4g+3 twice: one word of the
// data row per B fragment.
constexpr int MF_D = 12;
constexpr int MF_ROW_F16 = 28;
constexpr int MF_ROW_BYTES = 2 * MF_ROW_F16;
constexpr float MF_PAD_SCORE = 65504.0f;   // nhi = nlo = f16 max for padding code vectors

// Wide MFMA layout (every D != 12, Dp <= 64): per code vector KS k-steps of 32 f16 slots,
// [hi(DH) | lo(DH) | nhi nlo | 0 ...] with DH = Dp rounded up to 8 (hi/lo of components
// D..DH-1 are 0), same hi/lo/n meaning as above.
__host__ __device__ constexpr uint32_t wide_dh(uint32_t Dp) { return (Dp + 7) & ~7u; }
__host__ __device__ constexpr uint32_t wide_ks(uint32_t Dp) { return (2 * wide_dh(Dp) + 2 + 31) / 32; }
__host__ __device__ constexpr uint32_t wide_row_f16(uint32_t Dp) { return 32 * wide_ks(Dp); }
// f16 slots per code-vector row and the offset of the lo half, for either layout
__host__ __device__ inline uint32_t cb_row_f16(uint32_t D, uint32_t Dp) { return D == MF_D ? MF_ROW_F16 : wide_row_f16(Dp); }
__host__ __device__ inline uint32_t cb_lo_off(uint32_t D, uint32_t Dp) { return D == MF_D ? MF_D : wide_dh(Dp); }
// f16 slot of component d's hi and lo part in a row of either layout (norm: slots 2*LO, +1)
__host__ __device__ inline uint32_t cb_hi_slot(uint32_t D, uint32_t Dp, uint32_t d) {
    return D == MF_D ? 8 * (d / 4) + d % 4 : d;
}
__host__ __device__ inline uint32_t cb_lo_slot(uint32_t D, uint32_t Dp, uint32_t d) {
    return D == MF_D ? 8 * (d / 4) + 4 + d % 4 : wide_dh(Dp) + d;
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (each defined next to its kernel).  All take the stream last-but-args.
// ---------------------------------------------------------------------------------------
hipError_t launch_gen(hipStream_t s, uint8_t *rgb, uint32_t S, uint64_t seed0, uint64_t npix);
// Decode gather (CompressedImage::decompress): codebook bytes [K][D], A [wB*hB] -> raster [xs*ys*3].
// With orig (the original raster) the squared signed-byte differences are added to *sqerr.
hipError_t launch_decode(hipStream_t s, const uint8_t *cb, uint32_t K, uint32_t D, const uint32_t *A, uint32_t xs,
                         uint32_t ys, uint32_t w, uint32_t h, uint8_t *rgb, const uint8_t *orig, uint64_t *sqerr,
                         uint32_t *bad);
hipError_t launch_tile(hipStream_t s, const uint8_t *rgb, uint8_t *codes, uint32_t n_images, uint32_t xSize,
                       uint32_t ySize, uint32_t bw, uint32_t bh, uint32_t D, uint32_t Dp, uint8_t pad);
// VALU fp32 search for any Dp (multiple of 4, <= 64); codebook C32 [K][Dp].
// assign_valu_tile: code vectors per LDS tile (KT; K <= KT: the whole codebook, one tile).
uint32_t assign_valu_tile(uint32_t Dp, uint32_t K);
hipError_t launch_assign_valu(hipStream_t s, int num_cu, uint32_t Dp, const uint8_t *codes, uint64_t N,
                              const float *C32, uint32_t K, const float *lut32, float alpha, float beta, float gamma,
                              uint32_t *A, uint32_t *flags, unsigned *flag_cnt);
// MFMA f16 search for D = 12, optionally with the centroid sums fused (K <= mf_fuse_max_k()).
// Flag rule (distances, unscaled): second - best <= mfma + 2*(alpha*sqrt(second) + beta*second)
// + gamma, where `mfma` bounds the error of one MFMA score and the rest the fp32 direct-form
// recompute ("near-tie flags").
// A re-assigned row of the fused path (the search added its terms at its provisional index
// `from`): its packed terms (hi << 32 | lo, plut) go to slab G (xslab [d][k], xcnt [k]) at
// `to` and to slab G + 1 (xslab + K*D, xcnt + K; subtracted by the reduce) at `from`.
// Called by the lanes of one wave (lane < D does component lane).
__device__ inline void move_row_terms(const uint8_t *codes, uint32_t Dp, uint32_t D, uint32_t row, uint32_t from,
                                      uint32_t to, uint32_t K, uint64_t *xslab, uint32_t *xcnt, const uint64_t *plut,
                                      uint32_t lane) {
    if (lane < D) {
        const unsigned long long t = plut[codes[(uint64_t)row * Dp + lane]];
        atomicAdd((unsigned long long *)&xslab[(uint64_t)lane * K + to], t);
        atomicAdd((unsigned long long *)&xslab[(uint64_t)K * D + (uint64_t)lane * K + from], t);
    }
    if (lane == 0) {
        atomicAdd(&xcnt[to], 1u);
        atomicAdd(&xcnt[K + from], 1u);
    }
}

// The same move into a second copy of the final sums (layout hi[D][K] | lo[D][K] | cnt[K], u64,
// added mod 2^64 to copy 0 by the finalize): kd_reduce_kernel's ties, concurrent with the
// reduce of the slabs into copy 0.
__device__ inline void move_row_sums(const uint8_t *codes, uint32_t Dp, uint32_t D, uint32_t row, uint32_t from,
                                     uint32_t to, uint32_t K, uint64_t *xs, const uint64_t *plut, uint32_t lane) {
    const uint64_t KD = (uint64_t)K * D;
    if (lane < D) {
        const uint64_t t = plut[codes[(uint64_t)row * Dp + lane]];
        const unsigned long long hi = t >> 32, lo = t & 0xFFFFFFFFull;
        atomicAdd((unsigned long long *)&xs[(uint64_t)lane * K + to], hi);
        atomicAdd((unsigned long long *)&xs[KD + (uint64_t)lane * K + to], lo);
        atomicAdd((unsigned long long *)&xs[(uint64_t)lane * K + from], 0ull - hi);
        atomicAdd((unsigned long long *)&xs[KD + (uint64_t)lane * K + from], 0ull - lo);
    }
    if (lane == 0) {
        atomicAdd((unsigned long long *)&xs[2 * KD + to], 1ull);
        atomicAdd((unsigned long long *)&xs[2 * KD + from], ~0ull);
    }
}

// Column reduce of G slabs into sums (copy 0 of the final layout) by one 1024-thread block: 64
// columns, 16 waves each adding every 16th slab, combined through red (2 x 16 x 64 u64).  The
// last nsub slabs are subtracted (hi and lo separately: the corrections of re-assigned rows,
// whose terms the search had added at their provisional index); every total stays >= 0.
__device__ inline void reduce_columns_block(const uint64_t *__restrict__ part, const uint32_t *__restrict__ part_cnt,
                                            uint32_t G, uint32_t nsub, uint32_t K, uint32_t D,
                                            uint64_t *__restrict__ sums, uint32_t bid, uint64_t *red) {
    uint64_t(*red_hi)[64] = reinterpret_cast<uint64_t(*)[64]>(red);
    uint64_t(*red_lo)[64] = reinterpret_cast<uint64_t(*)[64]>(red + 16 * 64);
    const uint64_t KD = (uint64_t)K * D;
    const uint64_t col = (uint64_t)bid * 64 + (threadIdx.x & 63);
    const int sg = threadIdx.x >> 6;
    uint64_t hi = 0, lo = 0;
    if (col < KD) {
#pragma unroll 4
        for (uint32_t g = sg; g < G; g += 16) {
            const uint64_t p = part[g * KD + col];
            const uint64_t sgn = g < G - nsub ? 0 : ~0ull;   // x ^ sgn - sgn: +x or -x (mod 2^64)
            hi += ((p >> 32) ^ sgn) - sgn;
            lo += ((p & 0xFFFFFFFFull) ^ sgn) - sgn;
        }
    } else if (col < KD + K) {
#pragma unroll 4
        for (uint32_t g = sg; g < G; g += 16) {
            const uint64_t c = part_cnt[(uint64_t)g * K + (col - KD)];
            hi += g < G - nsub ? c : 0ull - c;
        }
    }
    red_hi[sg][threadIdx.x & 63] = hi;
    red_lo[sg][threadIdx.x & 63] = lo;
    __syncthreads();
    if (sg == 0) {
        for (int i = 1; i < 16; i++) {
            hi += red_hi[i][threadIdx.x];
            lo += red_lo[i][threadIdx.x];
        }
        if (col < KD) {
            sums[col] = hi;
            sums[KD + col] = lo;
        } else if (col < KD + K) {
            sums[2 * KD + (col - KD)] = hi;
        }
    }
}

// Rows the kd-tree answers: their best two fp64 distances are within tie_rel relative (ties of
// the reference's own arithmetic), or close enough that the reference's centroid bits -- which
// may differ from the exact sums' by tie_abs / (2 sqrt(D)) per component -- can decide them
// (DESIGN.md 3.8): |d' - d| <= tie_abs sqrt(d) + tie_abs^2 / 2 for each distance.
__host__ __device__ inline bool in_tie_band(double d1, double d2, double tie_rel, double tie_abs) {
    const double gap = d2 - d1;   // d2 = inf: one candidate only, never a tie
    const double band = tie_abs * (sqrt(d1) + sqrt(fmin(d2, 1e300))) + tie_abs * tie_abs;
    return gap <= tie_rel * d1 || gap <= band;
}

struct MfThresholds {
    float mfma, alpha, beta, gamma;
    float inv_scale;   // 2^-t
    float mu, sx;      // x = mu + w * sx
    // small-K scan (expanded fp32 scores): flag when second - best <= e0 + e1 * sum_d |w_d|
    float e0, e1;
    // the mfma bound for one row (k_mf32.hip): m0 + m1 * sum_d |w_d| <= mfma
    float m0, m1;
};
uint32_t mf_fuse_max_k();
bool mf_can_search(uint32_t K);
bool mf_small_search(uint32_t K);   // launch_assign_mfma: the small-K scan (given E32)
// K <= 32: expanded fp32 scores from E32 [Kp][16] = [c''(0..11) | n | 0 0 0] (the MFMA row's
// terms in fp32; padding rows n = 1e30).
// perm / tint (finalize's prune_order, K <= PRUNE_MAXK): the pruned tile order of the MFMA
// search (assign_mf32_kernel PRUNE); null: every tile in index order.
hipError_t launch_assign_mfma(hipStream_t s, int grid, bool fuse, const uint8_t *codes, uint64_t N,
                              const _Float16 *cb_rows, const float *E32, uint32_t K, const float *C32,
                              const uint64_t *plut,
                              const MfThresholds &th, uint32_t *A, uint32_t *flags, unsigned *flag_cnt,
                              uint64_t *part, uint32_t *part_cnt, const uint32_t *perm = nullptr,
                              const int32_t *tint = nullptr, uint64_t *z1 = nullptr, uint32_t nz1 = 0);
// (z1, nz1: fused searches also clear these nz1 u64 -- copy 1 of the final sums -- spread over the grid)
// The same search on v_mfma_f32_32x32x16_f16 tiles (k_mf32.hip); launch_assign_mfma uses it
// for K above the small-K scan whenever mf32_fits.
bool mf32_fits(uint32_t K, bool fuse);
bool mf32_prune_fits(uint32_t K, bool fuse);
// the fp32 codebook (the flagged rows' recompute) sits in LDS beside the MFMA rows
bool mf32_c32_staged(uint32_t K, bool fuse, bool prune);
hipError_t launch_assign_mf32(hipStream_t s, int grid, bool fuse, const uint8_t *codes, uint64_t N,
                              const _Float16 *cb_rows, uint32_t K, const float *C32, const uint64_t *plut,
                              const MfThresholds &th, uint32_t *A, uint32_t *flags, unsigned *flag_cnt,
                              uint64_t *part, uint32_t *part_cnt, const uint32_t *perm = nullptr,
                              const int32_t *tint = nullptr,
                              uint64_t *z1 = nullptr, uint32_t nz1 = 0);
constexpr uint32_t PRUNE_MAXK_HOST = 4096;   // prune_order's capacity (prune_order.hpp PRUNE_MAXK)
// d_tint: the envelopes (2 int32 per tile, PRUNE_MAXK_HOST / 32 tiles), then Kpad floats of
// projections (finalize -> prune_order)
inline size_t tint_bytes(uint32_t Kp) { return (size_t)2 * (PRUNE_MAXK_HOST / 32) * 4 + (size_t)Kp * 4; }
// MFMA f16 search for D != 12 (wide layout), no fused sums: K >= 32, codebook staged in LDS
// whole or in double-buffered slices.  Same flag rule as launch_assign_mfma.
// perm / tint (prune_order): the pruned variant for streamed codebooks (wide_prune_fits); cpr:
// 64-row chunks per image column of blocks (the workgroup's chunks stack across it; 1 = none).
bool wide_can_search(uint32_t Dp);
bool wide_prune_fits(uint32_t Dp, uint32_t K);
// the whole codebook sits in one workgroup's LDS (the search is not streamed)
bool wide_codebook_resident(uint32_t Dp, uint32_t K);
hipError_t launch_assign_wide(hipStream_t s, int num_cu, uint32_t Dp, uint32_t D, const uint8_t *codes, uint64_t N,
                              const _Float16 *cb_rows, uint32_t K, const float *C32, const MfThresholds &th,
                              uint32_t *A, uint32_t *flags, unsigned *flag_cnt, const uint32_t *perm = nullptr,
                              const int32_t *tint = nullptr, uint32_t cpr = 1, unsigned *sched = nullptr);
// (sched: two zeroed u32 the pruned variant's task counter uses and leaves zeroed)
// perm / tint / qscale = D / sx^2 (the level's pruned order; the chunked sweep only): only the
// positions the projection bound admits for the rows' fp32 bands are swept.
// Recheck of flagged rows: fp32 distances to all K code vectors (C32 [Kpad][Dp]), fp64 in
// the reference's order for those inside the fp32 error band (alpha, beta, gamma as the VALU
// search's); exact ties are listed in ties (tie_cnt) for launch_kd_resolve or the host.
// With xslab != nullptr adds every other row's packed terms (hi << 32 | lo) to xslab [d][k]
// and its count to xcnt [k] (the search's extra slab G).
// recheck_path: the fp32 codebook whole in LDS, swept in LDS chunks (Dp = 12, 48), or read from
// global memory.
enum class RecheckPath { Staged, Chunked, Global };
RecheckPath recheck_path(uint32_t Dp, uint32_t K);
hipError_t launch_recheck(hipStream_t s, int num_cu, const uint8_t *codes, uint32_t Dp, uint32_t D,
                          const uint32_t *flags, const unsigned *flag_cnt, const double *C64, const float *C32,
                          uint32_t K, const double *lut64, float alpha, float beta, float gamma, double tie_rel, double tie_abs,
                          uint32_t *A, uint32_t *ties, unsigned *tie_cnt, uint64_t *xslab, uint32_t *xcnt,
                          const uint64_t *plut,
                          const uint32_t *perm = nullptr, const int32_t *tint = nullptr, float qscale = 0.f);
// The recheck on the search's MFMA scores (D = 12, k_mf32.hip): same contract as launch_recheck
// (the band from th.m0 / th.m1), for K with recheck_mf32_fits.
bool recheck_mf32_fits(uint32_t K);
hipError_t launch_recheck_mf32(hipStream_t s, int num_cu, const uint8_t *codes, const uint32_t *flags,
                               const unsigned *flag_cnt, const _Float16 *cb_rows, const double *C64, uint32_t K,
                               const double *lut64, const MfThresholds &th, double tie_rel, double tie_abs, uint32_t *A,
                               uint32_t *ties, unsigned *tie_cnt, uint64_t *xslab, uint32_t *xcnt,
                               const uint64_t *plut);
// Device kd-tree answers for the listed ties (tree image in mapped host memory); adds their
// terms to sums when given.  kd_resolve_fits: the tree, stacks and one wave's point
// distances fit the LDS.
bool kd_resolve_fits(const KdView &kd, uint32_t K);
// kd_reduce_kernel: launch_kd_resolve (ties into copy 1 of sums) + launch_reduce (into copy 0).
// The reference kd-tree of P (K x D fp64, row-major) built on the device (k_kdbuild.hip), one
// workgroup: vind / nodes / nbox / cbox are scratch of K, 2K, 2K x 2D, 2K x 2D entries; flat gets
// kd_resolve's image (lo | hi | KdNodeDev[n] | vind, tree_bytes(K, D) at most), himg (mapped host
// memory, kdb_host_layout) the whole tree, its header's seq set to seq last.
bool kd_build_fits(uint32_t K, uint32_t D);
hipError_t launch_kd_build(hipStream_t s, const double *P, uint32_t K, uint32_t D, uint32_t *vind, KdbNode *nodes,
                           double *nbox, double *cbox, uint8_t *flat, uint8_t *himg, uint64_t seq);
bool kd_reduce_fits(const KdView &kd, uint32_t K);
hipError_t launch_kd_reduce(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, const uint32_t *ties,
                            const unsigned *tie_cnt, const double *C64, uint32_t K, const double *lut64,
                            const KdView &kd, uint32_t *A, const uint64_t *plut, const uint64_t *part,
                            const uint32_t *part_cnt, uint32_t G, uint32_t nsub, uint64_t *sums, uint64_t *sums1);
hipError_t launch_kd_resolve(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, const uint32_t *ties,
                             const unsigned *tie_cnt, const double *C64, uint32_t K, const double *lut64,
                             const KdView &kd, uint32_t *A, uint64_t *xslab, uint32_t *xcnt, const uint64_t *plut,
                             uint64_t *xsums = nullptr);   // xsums: moves into a final-sums copy (move_row_sums)
// update_plan: register runs into `copies` LDS replicas of the sums (update_runs_kernel), or
// `passes` passes of KR code vectors each over the rows (update_kernel); KR = 0: no room at all.
struct UpdatePlan {
    bool runs;
    uint32_t copies, KR, passes;
};
UpdatePlan update_plan(uint32_t K, uint32_t D);
hipError_t launch_update(hipStream_t s, uint32_t Dp, uint32_t G, const uint8_t *codes, uint64_t N, const uint32_t *A,
                         uint32_t K, uint32_t D, const uint64_t *plut, uint64_t *part, uint32_t *part_cnt);
// Sums of a final assignment straight into sums [hi KD][lo KD][cnt K] (no slabs, no reduce)
// through a counting sort of the rows by index: hist [G][K], scratch 2K + 1, idx / ks [N].
bool sorted_sums_fits(uint32_t K);
hipError_t launch_sorted_sums(hipStream_t s, uint32_t Dp, uint32_t G, const uint8_t *codes, uint64_t N,
                              const uint32_t *A, uint32_t K, uint32_t D, const uint64_t *plut, uint32_t *hist,
                              uint32_t *scratch, uint32_t *idx, uint32_t *ks, uint64_t *sums);
// A counter published to mapped host memory by a kernel: *dst = *cnt, then *flag = seq
// (flag null: nothing).
struct PubArgs {
    const unsigned *cnt = nullptr;
    uint32_t *dst = nullptr;
    uint64_t *flag = nullptr;
    uint64_t seq = 0;
};
// Sums of G slabs, the last nsub of them subtracted (fused path: slab G + 1 holds the terms
// of re-assigned rows at their provisional index).  pub: a tie count to publish first.
hipError_t launch_reduce(hipStream_t s, const uint64_t *part, const uint32_t *part_cnt, uint32_t G, uint32_t nsub,
                         uint32_t K, uint32_t D, uint64_t *sums, PubArgs pub = PubArgs());
// Up to three device ranges (sizes multiples of 4 bytes, 0 = unused) copied in one launch,
// e.g. into mapped pinned host memory; with flag (mapped) the copy then publishes *flag = seq
// (done: a block counter at 0, left at 0).
hipError_t launch_copy_out(hipStream_t s, const void *src0, void *dst0, uint64_t bytes0, const void *src1, void *dst1,
                           uint64_t bytes1, const void *src2, void *dst2, uint64_t bytes2, uint64_t *flag = nullptr,
                           uint64_t seq = 0, unsigned *done = nullptr);
// Mean sums (K = 1): block b adds into copy b mod MEAN_COPIES of [hi D][lo D][n] (stride
// 2D + 1; n in copy 0 only), so the blocks' closing atomics spread over MEAN_COPIES addresses
// per component; the K = 1 finalize adds the copies.  Also clears zero[0..n_zero) and sets
// dist[0] = sum ||x||^2 and dist[1] = rows from the byte histogram hist (values v64).
constexpr uint32_t MEAN_COPIES = 8;
hipError_t launch_mean_sums(hipStream_t s, uint32_t Dp, const uint8_t *codes, uint64_t N, uint32_t D,
                            const uint64_t *plut, uint64_t *sums, unsigned *zero, uint32_t n_zero, double *dist,
                            const uint64_t *hist, const double *v64);
// The level's tie rows exported with the codebook (the speculative Kahan check, engine.cpp):
// out (mapped host memory) = [u32 count][u32 pad] then per row [u32 row][u32 A[row]][Dp code
// bytes], the first cap rows; released with the ready flag.
struct TieExport {
    const uint32_t *rows = nullptr;
    const unsigned *cnt = nullptr;
    const uint32_t *A = nullptr;
    const uint8_t *codes = nullptr;
    uint32_t cap = 0;
    uint64_t n_rows = 0;   // rows in codes / A (a row index past it is written as ~0, nothing read)
    uint8_t *out = nullptr;
};
// The finalize (k_finalize.hip): one kernel, its form chosen by sums, children and measure:
//   sums, children 2:   C_cent = the exact centroids of the K cells; C_next (and host_cb, then the
//                       cells' row counts, u32) = the 2K split code vectors (x1.2 | x0.8), with
//                       their search tables padded to Kpad and, given perm / tint, their tile order
//                       (qvq_lbg's levels);
//   sums, children 1:   the same without the split: C_cent = C_next = the centroids, the tables of
//                       the same K (qvq_refine's centroid step);
//   no sums, children 1: the tables of the codebook C_src, whose values also go to C_next /
//                       host_cb where given (qvq_assign; qvq_refine's starting point);
//   sums, children 0:   C_cent only (qvq_update; qvq_lbg's last level);
//   sums, measure:      nothing written but the distortion term of the codebook C_src under sums
//                       that need not be its own (QVQ_REFINE_FRESH).
// The distortion term sum_k (2 c_k.S_k - n_k ||c_k||^2) (closed-form distortion) goes to
// dist_out[0] and its bits to pub[1].  With done the last block to finish clears what it is asked
// to, publishes pub[0..1] and then *ready = seq (pub, ready, host_cb and ties.out: mapped host
// memory); without done nothing of "the end" below happens.
struct FinArgs {
    // the cells
    const uint64_t *sums = nullptr;   // the reduced sums hi[d][k] | lo[d][k] | cnt[k]; null: rows from C_src
    uint32_t K = 0, D = 0, Dp = 0;
    int64_t R = 0, bias = 0;          // Terms
    int scale = 0;
    uint32_t ncopy = 1;               // copies of the sums to add: the mean's MEAN_COPIES, or 2 (kd_reduce_kernel)
    uint64_t cstride = 0;             // u64 from one copy to the next (0: they follow each other, 2KD + K apart)
    const unsigned *gate = nullptr;   // non-null: copies past the first only when *gate != 0 (the level's
                                      // tie count: without ties copy 1 is all zero, neither read nor cleared)
    bool zero_sums = false;           // the last block clears copies zero_skip .. ncopy - 1 (under the gate)
    uint32_t zero_skip = 0;
    // the rows
    uint32_t children = 0;            // table rows per cell: 2 the split, 1 the same K, 0 no tables
    uint32_t Kpad = 0;                // table rows in all: rows children K .. Kpad - 1 are padding that never wins
    const double *C_src = nullptr;    // sums == null: the codebook to prepare (children 2: K rows, split into
                                      // C_next's 2K); measure: the codebook measured
    bool measure = false;
    double *C_cent = nullptr;         // the centroids [K][D]
    double *C_next = nullptr;         // the table rows' code vectors [children K][D]: the next search's codebook
    double mu = 0, sx = 0;            // Terms
    int t = 0;                        // the MFMA scores' scale 2^t
    float *C32 = nullptr;             // fp32 [Kpad][Dp] (VALU path and the rechecks)
    _Float16 *rows = nullptr;         // the f16 MFMA rows (D = 12 or wide layout)
    float *E32 = nullptr;             // D = 12: expanded fp32 terms [c''(12) | n | 0 0 0] (small-K scan)
    double *host_cb = nullptr;        // mapped host memory: C_next's values for the host's kd-tree build
    uint32_t *perm = nullptr;         // the next search's tile order (prune_order), or null
    int32_t *tint = nullptr;
    TieExport ties;                   // out != null: the level's tie rows to mapped memory
    // the end
    double *dist_part = nullptr;      // per-block partials of the distortion term (512 doubles)
    unsigned *done = nullptr;         // block counter at 0, left at 0
    double *dist_out = nullptr;
    unsigned *changed = nullptr;      // launch_count_changed's total: published as pub[0] (null: 0), then cleared
    uint64_t *changed64 = nullptr;    // or (a communicator): the all-reduced total behind the level's sums
                                      // (launch_count_changed64), published and cleared the same way
    unsigned *clear_cnt = nullptr;    // the iteration's flag and tie counters (2), cleared for the next one
    uint64_t *pub = nullptr;          // [0] rows changed, [1] the distortion term's bits (0 without sums)
    uint64_t *ready = nullptr;
    uint64_t seq = 0;
};
hipError_t launch_finalize(hipStream_t s, const FinArgs &f);
// *out += the rows i < N with A[i] != B[i] (A, B 16-byte aligned).
hipError_t launch_count_changed(hipStream_t s, int num_cu, const uint32_t *A, const uint32_t *B, uint64_t N,
                                unsigned *out);
// The same into a u64 total: the slot behind a level's sums, all-reduced with them (qvq_refine on
// a communicator).
hipError_t launch_count_changed64(hipStream_t s, int num_cu, const uint32_t *A, const uint32_t *B, uint64_t N,
                                  uint64_t *out);
// *out (mapped host memory) = the cells k < K without a row under the reduced sums, their ncopy copies
// cstride apart added under the finalize's gate (qvq_lbg_lloyd's per-level count).
hipError_t launch_count_empty(hipStream_t s, const uint64_t *sums, uint32_t K, uint32_t D, uint32_t ncopy,
                              uint64_t cstride, const unsigned *gate, uint64_t *out);
// qvq_refine's empty-cell reseed (k_reseed.hip, reseed_rule.hpp; QVQ_REFINE_RESEED): scratch for K
// cells in one allocation of reseed_layout(K).total bytes (offsets in bytes; the donors' lists
// hold K rounded up to a power of two).
struct ReseedWork {
    unsigned *state = nullptr;     // [0] the iteration's empty cells (count adds, select clears)
    uint64_t *E = nullptr;         // [K] the cells' summed quantised errors
    uint64_t *far = nullptr;       // [K] the cells' far-row keys (reseed_far_key)
    uint64_t *dE = nullptr;        // the donors' E, then sorted
    uint32_t *cnt = nullptr;       // [K] the cells' rows
    uint32_t *empties = nullptr;   // [K] the empty cells, ascending
    uint32_t *dK = nullptr;        // the donors' cells
};
struct ReseedLayout {
    uint64_t E = 0, far = 0, dE = 0, cnt = 0, empties = 0, dK = 0, total = 0;
};
ReseedLayout reseed_layout(uint32_t K);
ReseedWork reseed_work(uint8_t *base, uint32_t K);
// The rows pass: a lane per row, RSD_THREADS lanes per block, at most RSD_GRID_CAP blocks (more
// rows: the grid-stride loop again).
constexpr int RSD_THREADS = 256;
constexpr int RSD_GRID_CAP = 512;
// The three launches, in this order after the reduce: count reads the cells' rows from the reduced
// sums (the finalize's copies, stride and gate: before the finalize that clears them) and leaves
// the number of empty cells in w.state; rows (after the centroid step wrote C) and select return at
// once when it is 0.  select writes the seeds into C and the number placed to *pub (mapped memory).
// N < 2^32 - 1.
hipError_t launch_reseed_count(hipStream_t s, const uint64_t *sums, uint32_t K, uint32_t D, uint32_t ncopy,
                               uint64_t cstride, const unsigned *gate, const ReseedWork &w);
hipError_t launch_reseed_rows(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N,
                              const uint32_t *A, const double *C, uint32_t K, const double *lut64, bool scaled,
                              const ReseedWork &w);
hipError_t launch_reseed_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N,
                                const double *lut64, double *C, uint32_t K, const ReseedWork &w, uint64_t *pub);
hipError_t launch_gather_codes(hipStream_t s, const uint8_t *codes, uint32_t Dp, const uint32_t *rows, uint32_t n,
                               uint8_t *out);
// qvq_median_cut (k_mediancut.hip, median_cut_rule.hpp, median_cut_plan.hpp): scratch for K = 2^bits
// boxes of D components in one allocation of mc_layout(K, D).total bytes (offsets in bytes).
struct McWork {
    uint32_t *cuts = nullptr;   // [32] boxes cut per level
    uint4 *sel = nullptr;       // [K/2] per box of the level: axis, lo, hi on it, t (or: not cut)
    uint32_t *lo = nullptr;     // [K][D] the boxes' minima of the row ordinals ...
    uint32_t *hi = nullptr;     // ... and maxima
    uint32_t *hist = nullptr;   // [K/2][256] the boxes' counts on their axis
};
struct McLayout {
    uint64_t cuts = 0, sel = 0, lo = 0, hi = 0, hist = 0, total = 0;
};
McLayout mc_layout(uint32_t K, uint32_t D);
McWork mc_work(uint8_t *base, uint32_t K, uint32_t D);
// A call: init; per level l (half = 2^(l-1) boxes): rows(half_prev = half / 2, ranges), axis(half),
// hist(half), cut(half, l); then rows(half_prev = K / 2, no ranges).  A holds the labels.
hipError_t launch_mc_init(hipStream_t s, uint32_t D, const McWork &w);
hipError_t launch_mc_rows(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N, uint32_t *A,
                          uint32_t half_prev, bool ranges, const McWork &w);
hipError_t launch_mc_axis(hipStream_t s, uint32_t boxes, uint32_t D, const McWork &w);
hipError_t launch_mc_hist(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t N, const uint32_t *A,
                          uint32_t boxes, const McWork &w);
hipError_t launch_mc_cut(hipStream_t s, uint32_t boxes, uint32_t D, uint32_t level, const McWork &w);
// qvq_kmeanspp (k_kmeanspp.hip, kmeanspp_rule.hpp, kmeanspp_plan.hpp): the call's own state.  All but
// m sit in one allocation of kmpp_layout(K, Dp).total bytes (offsets in bytes).
struct KmppWork {
    uint32_t *state = nullptr;       // [0] the stop flag (every row equals a seed), [1] placed
    uint32_t *seedw = nullptr;       // [16] the newest seed's code words as ordinals: the next update's input
    uint64_t *partial = nullptr;     // [KMPP_SEGMENTS_CAP] the segments' sums of m
    uint64_t *potential = nullptr;   // [K]
    uint32_t *rows = nullptr;        // [K] the seeds' rows
    uint32_t *seedcodes = nullptr;   // [K][Dp / 4] the seeds' code words as stored
    uint32_t *m = nullptr;           // [N] the rows' weight to their nearest seed (an allocation of its own)
};
struct KmppLayout {
    uint64_t seedw = 0, partial = 0, potential = 0, rows = 0, seedcodes = 0, total = 0;
};
KmppLayout kmpp_layout(uint32_t K, uint32_t Dp);
KmppWork kmpp_work(uint8_t *base, uint32_t *m, uint32_t K, uint32_t Dp);
// A call: init(row0 = the first seed); update(first); for j = 1 .. K - 1: select(j), update; select(K),
// which only publishes potential[K - 1].  After a select has raised the stop flag the rest return at once.
hipError_t launch_kmpp_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                            const KmppWork &w);
hipError_t launch_kmpp_update(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, bool first, const KmppWork &w);
hipError_t launch_kmpp_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t K,
                              uint64_t seed, const KmppWork &w);
// qvq_kmeanspp_greedy (k_kmeanspp_greedy.hip, kmeanspp_rule.hpp, kmeanspp_greedy_plan.hpp): the call's
// own state.  All but m sit in one allocation of kmppg_layout(K, Dp).total bytes.
struct KmppgWork {
    uint32_t *state = nullptr;             // [0] the stop flag, [1] placed, [2] the last published round's winning trial
    uint32_t *cand = nullptr;              // [2][16][16] the rounds' candidates as ordinals, by round parity
    uint32_t *candrow = nullptr;           // [2][16] ... and their rows
    uint64_t *part = nullptr;              // [16][KMPP_SEGMENTS_CAP] per trial, the segments' sums of min(m, w(., c_l))
    uint64_t *potential = nullptr;         // [K]
    uint64_t *trial_potential = nullptr;   // [K][16]
    uint32_t *rows = nullptr;              // [K] the seeds' rows
    uint32_t *trial = nullptr;             // [K] the winning trials
    uint32_t *trial_rows = nullptr;        // [K][16]
    uint32_t *seedcodes = nullptr;         // [K][Dp / 4] the seeds' code words as stored
    uint32_t *m = nullptr;                 // [N] the rows' weight to their nearest seed (an allocation of its own)
};
KmppgWork kmppg_work(uint8_t *base, uint32_t *m, uint32_t K, uint32_t Dp);
// A call with L trials: init(row0 = the first seed); evaluate(0, 1); for j = 1 .. K - 1: select(j),
// evaluate(j, L); select(K), which only publishes round K - 1.  evaluate(j) applies round j - 1's
// winner to m and sums every candidate of round j; select(j) publishes round j - 1 and draws round
// j's candidates, a block each.  After a select has raised the stop flag the rest return at once.
hipError_t launch_kmppg_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                             const KmppgWork &w);
hipError_t launch_kmppg_evaluate(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t L,
                                 const KmppgWork &w);
hipError_t launch_kmppg_select(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t j, uint32_t K,
                               uint32_t L, uint64_t seed, const KmppgWork &w);
// qvq_kmeans_par (k_kmeans_par.hip, kmeans_par_rule.hpp, kmeans_par_plan.hpp): the call's own state.
// All but m, near and mask sit in one allocation of kmpar_layout(K, Dp, plan).total bytes (offsets in
// bytes); the first 256 bytes are the state words and, from byte 96, potential[17].
struct KMeansParPlan;
struct KmparWork {
    uint32_t *state = nullptr;       // [0] the stop flag (phi = 0), [1] M, [2] [3] the newest candidates' range (first, count),
                                     // [4] rounds_run, [5] truncated, [6] placed, [8 .. 23] round_candidates
    uint64_t *potential = nullptr;   // [17]
    uint64_t *partial = nullptr;     // [KMPP_SEGMENTS_CAP] the segments' sums of m
    uint32_t *counts = nullptr;      // [KMPP_SEGMENTS_CAP] the segments' joining rows of the round ...
    uint32_t *offsets = nullptr;     // ... and their exclusive prefix
    uint32_t *cand_rows = nullptr;   // [max_candidates] the candidates' rows
    uint32_t *cand_wt = nullptr;     // [max_candidates] rows nearest to each
    uint32_t *cand_codes = nullptr;  // [max_candidates][Dp / 4] their code words as stored
    uint32_t *rows = nullptr;        // [K] the seeds' rows
    uint32_t *seedcodes = nullptr;   // [K][Dp / 4] the seeds' code words as stored
    uint32_t *gw = nullptr;          // [2][slots] the reduction's g and wt when they do not fit LDS
    uint32_t *slotcodes = nullptr;   // [slots][Dp / 4] ... and its lane-strided copy of the code words when they do not
    uint32_t *m = nullptr;           // [N] the rows' weight to their nearest candidate (an allocation of its own)
    uint32_t *near = nullptr;        // [N] ... and that candidate (an allocation of its own)
    uint64_t *mask = nullptr;        // [ceil(N / 64)] the round's joining rows, a bit each (an allocation of its own)
};
struct KmparLayout {
    uint64_t partial = 0, counts = 0, offsets = 0, cand_rows = 0, cand_wt = 0, rows = 0, cand_codes = 0, seedcodes = 0,
             gw = 0, slotcodes = 0, total = 0;
};
KmparLayout kmpar_layout(uint32_t K, uint32_t Dp, const KMeansParPlan &p);
KmparWork kmpar_work(uint8_t *base, uint32_t *m, uint32_t *near, uint64_t *mask, const KmparLayout &l);
// A call: init(row0 = candidate 0); update(first); for r = 1 .. rounds: sample(r) (count, scan, scatter),
// update; weights; reduce.  After a scan has raised the stop flag the rounds' launches return at once.
hipError_t launch_kmpar_init(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, uint32_t row0, uint32_t K,
                             const KMeansParPlan &p, const KmparLayout &l, const KmparWork &w);
hipError_t launch_kmpar_update(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               bool first, const KmparWork &w);
hipError_t launch_kmpar_sample(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               uint32_t r, uint64_t seed, const KmparWork &w);
hipError_t launch_kmpar_weights(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                                const KmparWork &w);
hipError_t launch_kmpar_reduce(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint64_t N, const KMeansParPlan &p,
                               uint32_t K, uint64_t seed, const KmparWork &w);
// Host-resolved rows: A[rows[i]] = vals[i]; with xslab their terms move from the
// provisional index (A before) to the new one (move_row_terms).
hipError_t launch_fix_rows(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint32_t *A,
                           const uint32_t *rows, const uint32_t *vals, uint32_t n, uint32_t K, uint64_t *xslab,
                           uint32_t *xcnt, const uint64_t *plut, uint64_t *xsums = nullptr);
// 256-bin histogram of the first D bytes of every row (hist zeroed first).
hipError_t launch_byte_hist(hipStream_t s, const uint8_t *codes, uint64_t N, uint32_t D, uint32_t Dp,
                            uint64_t *hist);
// The fp64 front door (k_ingest.hip, byte_image.hpp): X [n][dim] row-major, 8-byte aligned; tab
// [2][256] the spaces' Terms::v64, indexed by QVQ_CS_NORMAL / QVQ_CS_SCALED.  One lane per 4-byte
// code word, ING_THREADS lanes per block, at most ING_GRID_CAP blocks (more words: the grid-stride
// loop again).  classify: *verdict = the ING_* bits that hold for every value of the set (the
// launcher sets it first).  pack: codes [n][Dp] under colour space cs, pad bytes the space's pad code.
constexpr int ING_THREADS = 256;
constexpr int ING_GRID_CAP = 2048;
enum : unsigned { ING_SCALED_OK = 1, ING_NORMAL_OK = 2, ING_FINITE = 4 };
hipError_t launch_ingest_classify(hipStream_t s, const double *X, uint64_t n, uint32_t dim, const double *tab,
                                  unsigned *verdict);
hipError_t launch_ingest_pack(hipStream_t s, const double *X, uint64_t n, uint32_t dim, uint32_t cs, const double *tab,
                              uint8_t *codes);
// Rasters to exact mode's rows (k_tile64.hip, cie1931.hpp): launch_tile's tiling of n_images rasters,
// each pixel through the CIE1931 map, into X [N][3 * bw * bh] fp64 without padding.  One lane per
// (row, pixel in block) slot, T64_THREADS lanes per block, at most T64_GRID_CAP blocks (more slots:
// the grid-stride loop again).
constexpr int T64_THREADS = 256;
constexpr int T64_GRID_CAP = 2048;
hipError_t launch_tile64(hipStream_t s, const uint8_t *rgb, double *X, uint32_t n_images, uint32_t xSize,
                         uint32_t ySize, uint32_t bw, uint32_t bh);
// out [nrows][D] fp64 = lut64[code] of the first D bytes of rows row0 .. row0 + nrows - 1 of codes [.][Dp].
hipError_t launch_rows_f64(hipStream_t s, const uint8_t *codes, uint32_t Dp, uint32_t D, uint64_t row0, uint64_t nrows,
                           const double *lut64, double *out);
// Exact mode (k_exact.hip): fp64 rows X [N][D].
hipError_t launch_exact_assign(hipStream_t s, const double *X, uint64_t N, uint32_t D, const double *C, uint32_t K,
                               double tie_rel, uint32_t *A, uint32_t *ties, unsigned *tie_cnt);
size_t exact_sort_temp_bytes(uint64_t N);
hipError_t launch_exact_iota(hipStream_t s, uint32_t *v, uint64_t N);
// Kahan centroids of assignment A (nullptr: the mean of all rows, K = 1) into C [K][D] and
// counts cnt [K] (may be null); keys_out / order [N], koff [K + 1] and temp are scratch.
hipError_t launch_exact_centroids(hipStream_t s, const double *X, uint64_t N, uint32_t D, const uint32_t *A, uint32_t K,
                                  uint32_t *keys_out, uint32_t *iota, uint32_t *order, uint32_t *koff, void *temp,
                                  size_t temp_bytes, double *C, uint64_t *cnt);
hipError_t launch_exact_distortion(hipStream_t s, const double *X, uint64_t N, uint32_t D, const double *C,
                                   const uint32_t *A, double *part, double *out);
hipError_t launch_exact_gather(hipStream_t s, const double *X, uint32_t D, const uint32_t *rows, uint32_t n,
                               double *out);
hipError_t launch_exact_fix(hipStream_t s, uint32_t *A, const uint32_t *rows, const uint32_t *vals, uint32_t n);
// The reference's Kahan centroids on the device (k_kahan.hip, kahan_par.hpp): scratch for one
// computation over N rows and up to k_cap cells (sizes from KahanWork::caps).
struct KahanWork {
    uint32_t *hist = nullptr;          // [G][K] sort histograms (G = sort_blocks(N))
    uint32_t *tot = nullptr;           // [K] rows per cell
    uint32_t *koff = nullptr, *segoff = nullptr, *blkoff = nullptr;   // [K + 1] each
    uint8_t *planes = nullptr;         // [D][plane_len(N)]: the chains' bytes, component-major
    void *meta = nullptr;              // [D][seg_cap] segment metadata
    void *bsum = nullptr;              // [D][blk_cap] 128-bit block totals, then prefixes
    void *bfn = nullptr;               // [D][blk_cap] block functions
    void *sfn = nullptr;               // [D][seg_cap] segment functions
    void *bfn8 = nullptr;              // [D][blk_cap][8] 8-segment sub-block functions
    void *tab = nullptr;               // the byte table (kahan::ByteTab)
    unsigned *stats = nullptr;         // [4] blocks not composable, block misses, segment replays
    uint32_t n_one = 0;                // K = 1: N (the mean's single cell)
    uint64_t seg_cap = 0, blk_cap = 0, n_cap = 0;
    uint32_t k_cap = 0, d_cap = 0;
    static size_t tab_bytes();
    static void make_tab(const uint64_t *X, void *out);
    static void caps(uint64_t N, uint32_t K, uint64_t &segs, uint64_t &blks);
    static uint64_t plane_len(uint64_t N);
    static size_t meta_bytes();
    static size_t fn_bytes();
    static size_t segfn_bytes();
    static uint32_t sort_blocks(uint64_t N);
    // the sort's keys per launch window (its LDS counters) and the windows K keys take: any K sorts
    static uint32_t sort_window_keys();
    static uint32_t sort_windows(uint32_t K);
};
// C [K][D] = the reference's centroids of assignment A (nullptr: K = 1, the mean of every row):
// Kahan sums in ascending row order times fl(1/n), empty cells 0, bit for bit (SCALED byte
// values; w.tab from KahanWork::make_tab).  With split_out also the split [2K][D] (x1.2 | x0.8).
// sel (n_sel entries, device; nullptr: every cell): the selected cells only, compacted: sel[a] =
// slot + 1 for a selected cell a, 0 otherwise; K is then the number of slots, and C / split_out
// rows are slots (split_out: slot | K + slot).  The sort skips the other rows' bytes.
// max_rows: a bound on the rows of any cell summed (0: unknown); at most kahan_direct_max()
// rows, each chain runs step by step on one lane (ks_direct_kernel) instead of through the
// segment functions, whose set-up costs more than short chains.
hipError_t launch_kahan_centroids(hipStream_t s, const KahanWork &w, const uint8_t *codes, uint32_t Dp, uint32_t D,
                                  uint64_t N, const uint32_t *A, uint32_t K, double *C, double *split_out,
                                  const uint32_t *sel = nullptr, uint32_t n_sel = 0, uint64_t max_rows = 0);
uint64_t kahan_direct_max();   // QVQ_KAHAN_DIRECT_MAX (default 4096; 0: never)
// The same centroids when a cell's rows are split over ranks (each rank holds a contiguous
// range of the global rows, ranks in row order; engine.cpp kahan_chained).  gather: u64
// [nranks][K * D][2] chain totals | [nranks][K] row counts, zeroed by the caller; each rank
// writes its slice (chain_local) and the caller sums gather over the ranks (an all-gather);
// chain_build then takes each chain's exact prefix from the lower ranks' totals.  state: u64
// [K * D][2], the reference's (sum, c) bits: chain_eval (once per rank, in rank order, each from
// the previous rank's output; rank 0 from zeros) advances it over this rank's rows; chain_finish
// divides by the global row count (C [K][D], split_out [2K][D] as launch_kahan_centroids).
hipError_t launch_kahan_chain_local(hipStream_t s, const KahanWork &w, const uint8_t *codes, uint32_t Dp, uint32_t D,
                                    uint64_t N, const uint32_t *A, uint32_t K, const uint32_t *sel, uint32_t n_sel,
                                    uint64_t *gather, uint32_t rank, uint32_t nranks);
hipError_t launch_kahan_chain_build(hipStream_t s, const KahanWork &w, uint32_t D, uint64_t N, uint32_t K,
                                    const uint64_t *gather, uint32_t rank);
hipError_t launch_kahan_chain_eval(hipStream_t s, const KahanWork &w, uint32_t D, uint64_t N, uint32_t K,
                                   uint64_t *state, const uint64_t *gather, uint32_t rank);
hipError_t launch_kahan_chain_finish(hipStream_t s, uint32_t D, uint32_t K, const uint64_t *state,
                                     const uint64_t *gather, uint32_t nranks, double *C, double *split_out);
}  // namespace qvq
