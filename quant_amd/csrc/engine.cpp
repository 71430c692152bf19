// engine.cpp -- host side of the qvq engine: context, per-level schedule, kd-tree builds,
// RCCL exchange and the C ABI of include/qvq.h.  No kernels here.
//
// Per split level (LBGIterate, src/Quantizer.cpp:98-108, one effective Lloyd step), all on
// one stream with no host round trip:
//   D == 12, K <= mf_fuse_max_k():  search (fused exact sums) -> recheck -> kd_resolve
//                                   -> reduce -> [all-reduce] -> finalize+split+tables
//   otherwise:                      search (MFMA or VALU) -> recheck -> kd_resolve -> update
//                                   -> reduce -> [all-reduce] -> finalize+split+tables
// While the GPU runs a level's search, the host builds the reference kd-tree over that
// level's codebook (which the previous finalize wrote to mapped memory) for kd_resolve.  A
// tree too large for the kernel's LDS falls back to a synchronous host resolution of the tie
// rows (resolve_host_ties).  A quantize starts with the mean kernel and ends with one
// copy_out launch into mapped memory, whose completion flag the host polls.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <rccl/rccl.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <memory>
#include <unordered_map>
#include <vector>

#include "byte_image.hpp"
#include "cie1931.hpp"
#include "common.hpp"
#include "decode_plan.hpp"
#include "exact_plan.hpp"
#include "kdtree.hpp"
#include "kmeans_par_plan.hpp"
#include "kmeans_par_rule.hpp"
#include "kmeanspp_greedy_plan.hpp"
#include "kmeanspp_plan.hpp"
#include "mean_plan.hpp"
#include "kmeanspp_rule.hpp"
#include "median_cut_plan.hpp"
#include "median_cut_rule.hpp"
#include "owned.hpp"
#include "qvq.h"
#include "reseed_rule.hpp"
#include "wait.hpp"

namespace qvq {

// src/ColorSpace.cpp:4-6 (NORMAL) and :16-21 (SCALED, reciprocal multiply under fast-math)
static double cs_value(int cs, int b) {
    const double s = (double)(signed char)(unsigned char)b;
    return cs == QVQ_CS_NORMAL ? s : (s + 128.0) * (1.0 / 255);
}

bool make_terms(int cs, Terms &t) {
    if (cs != QVQ_CS_NORMAL && cs != QVQ_CS_SCALED) return false;
    const bool scaled = cs == QVQ_CS_SCALED;
    t.scale = scaled ? 60 : 0;
    t.vmax = 0;
    // u = (int8)b + 128 orders the bytes by value: SCALED v = fl(u * fl(1/255)),
    // NORMAL v = u - 128.  q = R*u + E with |E| <= 64 (SCALED) or E = -128 (NORMAL).
    t.R = scaled ? (int64_t)std::ldexp(1.0 / 255, 60) : 1;
    t.mu = scaled ? 0.5 : -0.5;
    t.sx = scaled ? (1.0 / 255) / 2 : 0.5;
    int64_t E[256], emax = 0;
    for (int b = 0; b < 256; b++) {
        t.v64[b] = cs_value(cs, b);
        t.v32[b] = (float)t.v64[b];
        t.vmax = std::max(t.vmax, std::fabs(t.v64[b]));
        const double qd = std::ldexp(t.v64[b], t.scale);
        if (qd != std::floor(qd)) return false;
        const int64_t u = (int64_t)(signed char)(unsigned char)b + 128;
        E[b] = (int64_t)qd - t.R * u;
        emax = std::max<int64_t>(emax, E[b] < 0 ? -E[b] : E[b]);
        t.hi[b] = (uint32_t)u;
        t.w[b] = (float)(2 * u - 255);   // v - mu = w * sx (exactly, up to fl() of v)
    }
    t.bias = emax;
    for (int b = 0; b < 256; b++) t.lo[b] = (uint32_t)(E[b] + t.bias);
    t.pad_code = scaled ? 0x80 : 0x00;
    return t.v64[t.pad_code] == 0.0;
}

}  // namespace qvq

using namespace qvq;

// d_counters: per level l < 33 [2l] flagged rows and [2l + 1] kd-tree ties; the block counters of the
// finalize's and of the hand-off copies' last-block publication; the pruned wide search's two task counters
constexpr uint32_t LEVEL_COUNTERS = 2 * 33, FIN_DONE_COUNTER = LEVEL_COUNTERS, COPY_DONE_COUNTER = LEVEL_COUNTERS + 1;
constexpr uint32_t SCHED_COUNTERS = LEVEL_COUNTERS + 2, N_COUNTERS = SCHED_COUNTERS + 2;
// ... and behind the counters a quantize clears: qvq_refine's rows-changed total (count_changed_kernel)
constexpr uint32_t CHANGED_COUNTER = N_COUNTERS, N_COUNTERS_ALLOC = N_COUNTERS + 2;
// Levels whose kd-tree the device builds (k_kdbuild.hip, beside the search): K * D from this up
// (C4's 48-D levels from K = 512; C3's 12-D trees take the host well under 0.1 ms).
constexpr uint64_t KDB_MIN_KD = 16384;

namespace qvq {
// One level's tie certificate (engine.cpp certify_rows): the level's distinct tie
// rows, the split as far as its reference bits are known, the answers; with several ranks the
// rows left open and the cells they need wait for the end of the quantize (cert_finish).
struct CertState {
    std::vector<double> qs;           // distinct tie rows (nu x D values)
    uint32_t nu = 0;
    std::vector<uint32_t> of;         // tie record -> distinct row
    std::vector<uint32_t> rows, spec; // the tie records: row, speculative index
    std::vector<double> kp;           // the reference's split where known
    std::vector<uint8_t> known;
    std::vector<int64_t> ans;         // per distinct row: the reference's index, -1 open
    std::vector<uint32_t> pend;       // distinct rows still open
    std::vector<uint8_t> sel;         // [K/2] the parent cells those rows need
    uint32_t cells = 0, rounds = 0;
    bool prepared = false;            // kp / known set and the tree's replay state built (cert_init)
};
}  // namespace qvq

// QVQ_HOST_TRACE=1: a host timeline of each qvq_lbg (us since its start, per thread), printed
// to stderr at its end: the main thread's tree builds and enqueues, the checks' start, export
// and end (diagnostics for where a quantize waits).  One per context: the checks of a context
// mark it from its worker thread while the calling thread does.
struct HostTrace {
    std::atomic<bool> on{false};
    std::chrono::steady_clock::time_point t0;
    std::mutex m;
    std::vector<std::pair<double, std::string>> ev;
    void start(std::chrono::steady_clock::time_point t) {
        std::lock_guard<std::mutex> g(m);
        t0 = t;
        ev.clear();
        on.store(true, std::memory_order_release);
    }
    void mark(const std::string &what) {
        if (!on.load(std::memory_order_acquire)) return;
        std::lock_guard<std::mutex> g(m);
        const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ev.emplace_back(t, what);
    }
    std::string finish() {
        std::lock_guard<std::mutex> g(m);
        on.store(false, std::memory_order_release);
        // (t0 in steady_clock ns -- CLOCK_MONOTONIC, the clock of rocprofv3's timestamps)
        std::string out = "qvq host trace: t0_ns " +
                          std::to_string(std::chrono::duration_cast<std::chrono::nanoseconds>(t0.time_since_epoch()).count());
        for (const auto &e : ev) out += "\n  " + std::to_string((int)e.first) + " " + e.second;
        return out;
    }
};

// The context owns its device memory, pinned memory, streams and events through the handles of
// owned.hpp, grouped by lifetime: what is made with the context, the training set
// (ts), the level buffers of one Kcap (lv), the Kahan state (kh) and scratch that only grows.  A
// group is rebuilt in a local and moved in when every allocation has succeeded, and dropped by
// assigning an empty one.  Members are destroyed in reverse order: the streams come first.
struct qvq_ctx {
    int dev = 0;
    int num_cu = 256;
    std::string err;
    // stream: every call's work; kstream: the device tree build (first use: ensure_levels);
    // vstream: the speculative check's selected Kahan sums (first use: ensure_speculation)
    Stream stream, kstream, vstream;

    // ---- made with the context (qvq_create), kept to qvq_destroy
    DevBuf<float> d_lut32, d_w;   // the resident colour space's tables (alloc_training uploads them)
    DevBuf<double> d_lut64;
    DevBuf<uint64_t> d_plut;
    DevBuf<unsigned> d_counters;   // per level: [2l] flagged rows, [2l+1] kd-tree ties; [66], [67] block counters;
                                   // [68], [69] the pruned wide search's task counters (SCHED_COUNTERS)
    DevBuf<uint64_t> d_hist;       // byte histogram [256] | its all-reduced copy [256]
    DevBuf<double> d_dist_part;
    DevBuf<uint64_t> d_mean;   // MEAN_COPIES x mean sums [hi D][lo D][n]: zero between quantizes (the finalize clears them)
    DevBuf<uint64_t> d_decode_stat;      // decode: [squared error, bad-index flag]
    PinnedBuf<uint64_t> h_decode_stat;   // pinned host copy
    // mapped, coherent: [0, 64) the codebook ready number, [64, 1024) a quantize's small results
    CoherentBuf<uint64_t> h_ready;
    Event ev[32][4], ev_end;
    Event ev_sync;   // wait_stream
    Event ev_kcb, ev_kdb;   // the device tree build's (first use: ensure_levels)
    // the fp64 front door (k_ingest.hip): both spaces' value tables [2][256], the classify pass's
    // verdict and its pinned copy; events around the passes and their device ms (qvq_set_timing(-3))
    DevBuf<double> d_ing_tab;
    DevBuf<unsigned> d_ing_verdict;
    PinnedBuf<unsigned> h_ing_verdict;
    Event ev_ing[3];
    double ingest_ms[2] = {0, 0};
    uint32_t G = 0;   // workgroup slabs
    // the speculative check's tie exports (TieExport, level % 3), mapped; made once (ensure_speculation)
    MappedBuf<uint8_t> h_tx[3];
    uint32_t tx_cap = 0;

    // ---- the training set: replaced as a whole by alloc_training / install_exact (N == 0: none)
    struct Training {
        uint64_t N = 0;
        uint32_t D = 0, Dp = 0;
        int cs = -1;
        Terms terms;
        int mf_t = 0;            // MFMA score scale exponent
        MfThresholds mf_th{};
        double tie_abs = 0;      // the recheck's absolute tie band: centroid bits may differ by this much
        DevBuf<uint8_t> d_codes;
        DevBuf<uint32_t> d_flags, d_ties;
        DevBuf<uint32_t> d_sortbuf;   // sorted-order sums: idx [N] | ks [N] (first use: run_update_slabs)
        // The assignment buffers, N indices each, grown by ensure_apool: one with the set, a second
        // for the previous level's assignment (Kahan levels, qvq_refine), four for the speculative
        // check, one per level with several ranks.
        std::vector<DevBuf<uint32_t>> apool;
        // Views of apool that qvq_lbg and qvq_refine rotate: d_A the current assignment, d_A_alt the
        // previous level's (the input of the reference-bit centroids a level with kd-tree ties
        // needs), d_A3 / d_A4 the two levels the speculative check still reads
        uint32_t *d_A = nullptr, *d_A_alt = nullptr, *d_A3 = nullptr, *d_A4 = nullptr;
        // exact mode (qvq_set_vectors_exact, or qvq_set_vectors on values that are not byte images):
        // the fp64 rows themselves and the reference's Kahan arithmetic (k_exact.hip)
        bool exact = false;
        int exact_cs = -1;   // the colour space whose raster the exact rows came from (QVQ_CS_CIE1931), -1: fp64 rows
        struct Exact {
            DevBuf<double> d_X64;
            DevBuf<uint32_t> d_keys, d_iota, d_order, d_koff;
            DevBuf<uint8_t> d_temp;
            size_t temp_bytes = 0;
        } ex;
        // qvq_kmeanspp's own state, cached between calls: m [N] and the work of kmpp_layout for up
        // to K seeds.  Part of the training set, so whatever replaces the set drops it.
        struct KMeansPP {
            DevBuf<uint32_t> d_m;
            DevBuf<uint8_t> d_work;
            uint32_t K = 0;
        } kpp;
        // qvq_kmeanspp_greedy's own state, cached between calls: m [N] and the work of kmppg_layout
        // (at least work_bytes).  Part of the training set as well.
        struct KMeansPPGreedy {
            DevBuf<uint32_t> d_m;
            DevBuf<uint8_t> d_work;
            uint64_t work_bytes = 0;
        } kppg;
        // qvq_kmeans_par's own state, cached between calls: m, near [N], the rounds' join bits and the
        // work of kmpar_layout (at least work_bytes).  Part of the training set as well.
        struct KMeansPar {
            DevBuf<uint32_t> d_m, d_near;
            DevBuf<uint64_t> d_mask;
            DevBuf<uint8_t> d_work;
        } kpar;
    } ts;

    // ---- level buffers for up to Kcap code vectors: replaced as a whole by ensure_levels
    struct Levels {
        uint32_t Kcap = 0;
        DevBuf<double> d_C64_cent, d_C64_split;
        DevBuf<double> d_C64_split_alt;   // qvq_lbg's next split while d_C64_split may still be needed
        DevBuf<float> d_C32;
        DevBuf<float> d_E32;   // D = 12: expanded fp32 terms for the small-K scan
        DevBuf<_Float16> d_rows;   // MFMA code-vector rows
        DevBuf<uint32_t> d_perm;   // pruned search: tile order of the split codebook (finalize's prune_order)
        DevBuf<int32_t> d_tint;    // ... and the tiles' projection envelopes
        uint32_t perm_k = 0;       // the K whose order d_perm holds (0: none)
        DevBuf<uint64_t> d_part, d_sums;
        DevBuf<uint32_t> d_part_cnt;
        // mapped pinned host memory (coherent): the split codebooks the finalizes publish for the
        // host, two halves of cb_half doubles (host_cb_of): level L's codebook in half L & 1;
        // two flattened kd-tree images
        CoherentBuf<double> h_cb;
        uint64_t cb_half = 0;
        CoherentBuf<uint8_t> h_tree[2];
        DevBuf<uint8_t> d_tree;   // device copy of the level's tree image (one DMA per level)
        uint64_t tree_cap = 0;
        // the level's kd-tree built on the device (k_kdbuild.hip) on kstream, beside the search:
        // scratch (vind, nodes, boxes) and the mapped host image of the whole tree
        DevBuf<uint32_t> d_kdb_vind;
        DevBuf<KdbNode> d_kdb_nodes;
        DevBuf<double> d_kdb_nbox, d_kdb_cbox;
        CoherentBuf<uint8_t> h_kdb;
        uint32_t kdb_cap = 0;   // code vectors the scratch takes (0: none)
    } lv;
    uint64_t seq = 0;
    uint64_t kdb_seq = 0;         // the device tree build's launch number
    uint64_t out_seq = 0;         // quantizes whose results copy_out has published
    uint64_t pub_seq = 0;         // per-level tie-count publications (h_ready[1] = seq, h_ready[2] = ties)
    // copy 1 of d_sums may hold moves that no finalize has taken (a call that stopped between the
    // two): raised by mark_sums1, lowered by run_finalize and clear_dirty_sums, nowhere else
    bool sums1_dirty = false;

    // ---- Kahan state of the training set: dropped with it, rebuilt in parts by ensure_kahan
    struct Kahan {
        struct Cells {   // for up to kcap cells
            uint32_t kcap = 0;
            DevBuf<double> d_kc_cent, d_kc_split;   // Kahan centroids [K/2][D], their split [K][D]
            DevBuf<uint32_t> d_kc_sel;     // [K/2] slot + 1 of the cells a tie certificate sums (0: not summed)
            PinnedBuf<uint32_t> h_kc_sel;  // its pinned host side
            MappedBuf<double> h_kc_out;    // [K][D] mapped: the selected cells' split rows
        } cells;
        struct Work {   // what kw views (common.hpp KahanWork, the launch wrappers' plain struct)
            DevBuf<uint32_t> hist, tot, koff, segoff, blkoff;
            DevBuf<uint8_t> planes, meta, bsum, bfn, sfn, bfn8, tab;
            DevBuf<unsigned> stats;
        } work;
        KahanWork kw;   // view of work, and its capacities
        DevBuf<uint64_t> d_kc_chain;   // chained Kahan sums: gather | state (k_kahan.hip), grown on demand
        uint32_t last_route = 0;       // qvq_get_kahan_stats: the last qvq_update_kahan* call's route
        // several ranks: the checks whose rows wait for cells summed over every rank's rows (status
        // 2), finished together at the end of qvq_lbg; A_prev stays valid (one assignment buffer per level)
        struct Deferred {
            uint32_t level = 0, K = 0;
            const uint32_t *A_prev = nullptr;   // view of an apool buffer
            std::unique_ptr<RefKDTree> tree;
            std::vector<double> cb;
            CertState cs;
        };
        std::vector<Deferred> deferred;
    } kh;
    std::vector<double> h_kc_split;   // host copy of the split for the tree build
    std::vector<double> cert_kp;      // the reference's split where known (tie certificate)
    std::vector<uint8_t> cert_known;
    std::vector<uint32_t> cert_vals;  // the certified answers (host side of their upload)

    // ---- scratch, grown on demand (ensure) and kept to qvq_destroy
    DevBuf<uint32_t> d_scatter;          // the host-resolved tie rows' uploads
    DevBuf<uint8_t> d_raster;            // qvq_set_images' raster upload buffer
    DevBuf<uint8_t> d_decode;            // qvq_decode's and qvq_get_vectors' scratch
    DevBuf<uint8_t> d_reseed;            // QVQ_REFINE_RESEED's scratch (reseed_layout)
    // qvq_median_cut's scratch (mc_layout) for K boxes of D components: built in a local of this
    // type and moved here once every allocation of the call has succeeded
    struct MedianCut {
        DevBuf<uint8_t> d_work;
        uint32_t K = 0, D = 0;
    } mc;
    DevBuf<uint64_t> d_vote;             // the ranks' small all-reduced decisions (qvq_lbg)
    PinnedBuf<uint64_t> h_vote;
    PinnedBuf<uint8_t> h_ar_stage;       // pinned staging of the host all-reduce
    PinnedBuf<uint8_t> h_stage;          // pinned staging of qvq_update's results

    std::vector<double> cb_local;   // host copy of the published codebook for the tree build
    std::vector<uint32_t> cnt_local;   // ... and of its parent cells' row counts (empty: not known)
    std::unique_ptr<RefKDTree> tree;   // the last level's tree over cb_local
    KdView tree_kd;                    // and its device image: a view of lv.d_tree or lv.h_tree[] (depth 0: none)
    // deferred-tie levels build their tree on this worker, off the launch path (start_tree_job)
    struct Worker {   // one host thread, jobs in order
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::function<void()>> q;
        bool stop = false;
        std::atomic<int> pending{0};
    } worker;
    // helpers of the worker for the certificate's replays (persistent: their per-thread replay
    // caches stay warm); pool_run forks fn over them and the calling thread
    struct Pool {
        std::vector<std::thread> th;
        std::mutex m;
        std::condition_variable cv;
        std::function<void(uint32_t)> fn;
        std::atomic<uint64_t> epoch{0};
        std::atomic<uint32_t> want{0}, busy{0};
        std::atomic<bool> stop{false};
    } pool;
    // one rank: the CPUs of the L3 domain the first quantize ran on (host_place)
    bool place_tried = false, place_ok = false;
    cpu_set_t place;
    // the speculative Kahan check (qvq_lbg): level L's ties verified on the worker while the GPU
    // runs levels L + 1 and L + 2; four assignment buffers keep A_{L-1} (the check's cells)
    // until level L + 3, when the check is joined
    struct Verify {
        bool posted = false;
        std::atomic<bool> done{true}, cancel{false};
        int status = 0;   // 0: the reference's indices are the speculative ones; 1: not shown; 2: deferred
        uint32_t K = 0, level = 0;
        uint64_t seq = 0;
        int par = 0;
        const uint32_t *A_prev = nullptr;   // view of an apool buffer
        std::unique_ptr<RefKDTree> tree;
        std::vector<double> cb;
        std::vector<uint32_t> cnt;   // the parent cells' row counts (empty: not known)
        CertState cs;
        Event ev;   // made once (ensure_speculation)
    } ver[3];   // level % 3
    std::atomic<bool> tree_cancel{false};
    bool tree_job = false, job_ok = false;
    int job_buf = 0;
    KdView job_kd;   // the tree job's image: a view of lv.h_tree[job_buf]
    uint32_t col_blocks = 0;   // blocks per image column (consecutive rows run down a column); 0: no image
    int timing_level = -2;   // qvq_set_timing: -1 all levels, -2 none (default), else that level only
    double timeout_s = 120;         // bound of every host wait (qvq_set_timeout, QVQ_TIMEOUT_S)

    // multi-GPU: an RCCL communicator, or (tests) a host all-reduce callback
    ncclComm_t comm = nullptr;
    qvq_allreduce_fn host_ar = nullptr;
    void *host_ar_user = nullptr;   // the caller's, passed back to host_ar
    int nranks = 1, rank = 0;
    // a bounded wait failed while work may still be queued on the stream: every later call
    // returns QVQ_ESTATE until qvq_destroy (results must not land in freed memory,
    // and the stream's scratch must not be reused under running kernels)
    bool poisoned = false;

    // qvq_refine's starting point when it is given none: the last successful qvq_lbg or qvq_refine
    // on the resident rows (K code vectors in d_C64_cent, their assignment in d_A, its distortion);
    // any other call that touches those buffers ends it.  xsq / rows: sum ||x||^2 and the row count
    // of the resident rows (from the byte histogram, once per training set)
    struct RefineState {
        bool valid = false;
        uint32_t K = 0;
        double dist = 0;
        bool have_xsq = false;
        double xsq = 0, rows = 0;
        // the last qvq_refine's seeds placed per iteration (all 0 without QVQ_REFINE_RESEED)
        bool have_reseeds = false;
        std::vector<uint64_t> reseeds;
    } rf;

    qvq_timings tm;
    HostTrace htrace;
};

namespace {

thread_local std::string g_static_err;

qvq_status fail(qvq_ctx *c, qvq_status st, const std::string &msg) {
    if (c) c->err = msg;
    else g_static_err = msg;
    return st;
}

// Entry points that use the device refuse a poisoned context (wait_failed).
#define GUARD(ctx)                                                                                    \
    do {                                                                                              \
        if (!(ctx)) return QVQ_EINVAL;                                                                \
        if ((ctx)->poisoned)                                                                          \
            return fail((ctx), QVQ_ESTATE, "context poisoned by an earlier failed wait; destroy it"); \
    } while (0)

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(ctx, QVQ_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

#define NCCLCHK(expr)                                                                                 \
    do {                                                                                              \
        ncclResult_t r_ = (expr);                                                                     \
        if (r_ != ncclSuccess)                                                                        \
            return fail(ctx, QVQ_ECOMM, std::string(#expr) + ": " + ncclGetErrorString(r_));          \
    } while (0)

uint32_t pad32(uint32_t K) { return (K + 31) & ~31u; }   // MFMA tile pairs
bool env_is(const char *name, const char *val) {
    const char *v = std::getenv(name);
    return v && std::strcmp(v, val) == 0;
}

// The dispatch of one level (N rows of D components, Dp padded, against K code vectors), decided
// once by plan_level: run_level and the finalize builders switch on it, qvq_host_plan reports it
// (DESIGN.md 6.1).  What depends on the call and not on the shape (sums wanted, the tile order at
// hand, a communicator, deferred ties) meets the plan at the top of run_level.
struct LevelPlan {
    uint32_t search = QVQ_PLAN_SEARCH_VALU;   // QVQ_PLAN_SEARCH_* (qvq.h)
    bool fusable = false;        // the sums can ride in the search (MFMA, K <= mf_fuse_max_k())
    bool prunable = false;       // the finalize before this level writes its tile order
    bool c32_staged = false;     // MF32: fp32 codebook in LDS when the search runs unfused, unpruned
    bool cb_resident = false;    // WIDE: whole codebook in LDS
    uint32_t valu_tiles = 0;     // VALU: codebook tiles
    uint32_t recheck = 0;        // QVQ_PLAN_RECHECK_*: the MFMA recheck, or launch_recheck's path
    bool sorted_sums = false;    // the sums pass through the counting sort; else update, launch_update's plan
    UpdatePlan update{};
    bool kd_host = false, kd_device = false;   // QVQ_KDTREE=host: no tree image; =device: the device build
    bool tree_shape = false;     // a shape the device build takes and is worth a launch for
    bool mfma() const { return search == QVQ_PLAN_SEARCH_SMALL || search == QVQ_PLAN_SEARCH_MF32; }
};
// MFMA search for D != 12 from K = 128 code vectors up: below it the VALU search wins (C4,
// D = 48: 82 vs 182 us at K = 32, 154 vs 187 at K = 64; from K = 64 or 32 the C4 levels ran
// slower, profiles/r05ak).
constexpr uint32_t WIDE_MIN_K = 128;
// Pruned MFMA search (k_mf32.hip PRUNE: tiles outside a chunk's provable window skipped) for
// D = 12 from K = 256 (from K = 128 it measured slower, profiles/r05ao) up to prune_order's
// capacity.  Its order is computed by the previous level's finalize.  Other D
// (assign_wide_kernel, streamed codebooks): from K = 1024; a codebook resident in LDS (small D)
// is searched unpruned: its per-wave windows measured no faster.
// The D = 12 kernel keeps one tile envelope per lane: at most 64 tiles (K <= 2048).
constexpr uint32_t PRUNE_MIN_K = 256, WPRUNE_MIN_K = 1024;
// The path knobs a test exercises are read here, at every call (tests flip them between calls):
// QVQ_SEARCH=valu (the VALU search at every K), QVQ_KDTREE=host (ties answered on the host) and
// QVQ_KDTREE=device (the level's tree built on the device, k_kdbuild.hip: opt-in, bit-identical
// to the host build but slower than it -- K = 4096 3.7 ms vs 1.8 ms, K = 2048 2.2 vs 0.7: a node
// costs ~10-20 us of dependent device round trips and barriers, and C4's trees have ~300 big
// nodes on one serial path -- so the host build, overlapping the search, stays the default,
// DESIGN.md 8).  The other knobs: QVQ_KAHAN=0 / QVQ_SPECULATE=0 (index rule and schedule,
// DESIGN.md 3.8-3.9); QVQ_KAHAN_FAIL_LEVEL / _RANK (forced check failures).
LevelPlan plan_level(uint32_t D, uint32_t Dp, uint64_t N, uint32_t K) {
    LevelPlan p;
    const bool valu = env_is("QVQ_SEARCH", "valu");
    p.kd_host = env_is("QVQ_KDTREE", "host");
    p.kd_device = env_is("QVQ_KDTREE", "device");
    const RecheckPath rp = recheck_path(Dp, K);
    p.recheck = rp == RecheckPath::Staged    ? QVQ_PLAN_RECHECK_STAGED
                : rp == RecheckPath::Chunked ? QVQ_PLAN_RECHECK_CHUNKED
                                             : QVQ_PLAN_RECHECK_GLOBAL;
    if (D == MF_D && mf_can_search(K) && !valu) {
        p.search = mf_small_search(K) ? QVQ_PLAN_SEARCH_SMALL : QVQ_PLAN_SEARCH_MF32;
        p.fusable = K <= mf_fuse_max_k();
        p.c32_staged = p.search == QVQ_PLAN_SEARCH_MF32 && mf32_c32_staged(K, false, false);
        p.prunable = K >= PRUNE_MIN_K && K <= 2048 && mf32_prune_fits(K, p.fusable);
        // the MFMA recheck from K = 512 (below it the fp32 pass over K code vectors is cheaper
        // than staging the MFMA tables, profiles/r02f)
        if (K >= 512 && recheck_mf32_fits(K)) p.recheck = QVQ_PLAN_RECHECK_MF32;
    } else if (D != MF_D && wide_can_search(Dp) && K >= WIDE_MIN_K && !valu) {
        p.search = QVQ_PLAN_SEARCH_WIDE;
        p.cb_resident = wide_codebook_resident(Dp, K);
        p.prunable = !p.cb_resident && K >= WPRUNE_MIN_K && K <= PRUNE_MAXK_HOST && wide_prune_fits(Dp, K);
    } else {
        const uint32_t KT = assign_valu_tile(Dp, K);
        p.valu_tiles = (K + KT - 1) / KT;
    }
    // sums of a final assignment through the counting sort (k_misc.hip) from K * D = 1536 (C4 from
    // K = 32: 5.52 -> 5.23 ms against 16384)
    p.sorted_sums = (uint64_t)K * D >= 1536 && sorted_sums_fits(K) && N <= 0xFFFFFFFFull;
    p.update = update_plan(K, D);
    // levels whose tree the device build takes (its LDS arrays) and is worth a launch for
    p.tree_shape = kd_build_fits(K, D) && (uint64_t)K * D >= KDB_MIN_KD;
    return p;
}
LevelPlan plan_level(const qvq_ctx *ctx, uint32_t K) { return plan_level(ctx->ts.D, ctx->ts.Dp, ctx->ts.N, K); }

// Flattened tree: root box lo[D], hi[D] | nodes[<= 2K] | vind[K].
uint64_t tree_bytes(uint32_t K, uint32_t D) {
    return 16ull * D + (2ull * K + 1) * sizeof(KdNodeDev) + 4ull * K;
}

// The range [cmin, cmax] of a code vector's components that the near-tie bounds below are worked
// out for: centroids are means of data values in [vmin, vmax], the split scales them by 1.2 or 0.8.
// qvq_assign refuses a byte-path codebook outside it.
void codebook_range(const Terms &t, double &vmin, double &vmax, double &cmin, double &cmax) {
    vmin = 1e300, vmax = -1e300;
    for (int b = 0; b < 256; b++) {
        vmin = std::min(vmin, t.v64[b]);
        vmax = std::max(vmax, t.v64[b]);
    }
    cmin = std::min(1.2 * vmin, 0.8 * vmin);
    cmax = std::max(1.2 * vmax, 0.8 * vmax);
}

// MFMA score scale and error bounds for the near-tie flag ("near-tie flags").
void mfma_setup(qvq_ctx::Training &ts) {
    const Terms &t = ts.terms;
    const double D = ts.D;
    double vmin, vmax, cmin, cmax, wmax = 0;
    codebook_range(t, vmin, vmax, cmin, cmax);
    for (int b = 0; b < 256; b++) wmax = std::max(wmax, (double)std::fabs(t.w[b]));
    const double cp = std::max(std::fabs(cmin - t.mu), std::fabs(cmax - t.mu));   // max |c - mu|
    const double n_max = D * cp * cp;
    const double c2_max = 2 * t.sx * cp;
    const double s_bound = n_max + D * wmax * c2_max;    // sum of |terms| of one score, unscaled
    int tt = 0;
    while (std::ldexp(n_max, tt + 1) <= 60000.0 && std::ldexp(s_bound, tt + 1) <= 120000.0) tt++;
    while (std::ldexp(n_max, tt) > 60000.0 || std::ldexp(s_bound, tt) > 120000.0) tt--;
    ts.mf_t = tt;
    const double u = std::ldexp(1.0, -24);
    // one MFMA score: <= (slots + 1) sequential fp32 roundings over the terms (D = 12: 32
    // slots in one MFMA; wide layout: KS chained MFMAs of 32 slots), the f16 hi/lo split
    // (2^-22 relative + 2^-25 absolute per operand, scaled back), the fp32 scale/shift of
    // the score and of ||x - mu||^2, x ~ mu + w*sx (2^-53)
    const double rounds = ts.D == MF_D ? 33.0 : 32.0 * wide_ks(ts.Dp) + 1.0;
    const double e_acc = rounds * u * s_bound;
    const double e_rep = D * wmax * (c2_max * std::ldexp(1.0, -22) + std::ldexp(1.0, -25 - tt)) +
                         n_max * std::ldexp(1.0, -22) + std::ldexp(1.0, -25 - tt);
    const double e_conv = 4 * u * (s_bound + D * cp * cp) + 1e-12 * s_bound;
    ts.mf_th.mfma = (float)(1.25 * (e_acc + e_rep + e_conv));
    // The same bound for one row, with sum_d |w_d| of that row in place of D * wmax (every term
    // above is linear in it): S_row = n_max + c2_max * sum|w| replaces s_bound.
    {
        const double ew = std::ldexp(1.0, -25 - tt);
        const double a0 = rounds * u * n_max + (n_max * std::ldexp(1.0, -22) + ew) + 4 * u * (n_max + D * cp * cp) +
                          1e-12 * n_max;
        const double a1 = rounds * u * c2_max + (c2_max * std::ldexp(1.0, -22) + ew) + 4 * u * c2_max + 1e-12 * c2_max;
        ts.mf_th.m0 = (float)(1.25 * a0 * 1.0001);
        ts.mf_th.m1 = (float)(1.25 * a1 * 1.0001);
    }
    // direct-form fp32 recompute (same bound as the VALU search)
    const double L = std::sqrt(D) * (std::max(std::fabs(vmin), std::fabs(vmax)) + std::max(std::fabs(cmin), std::fabs(cmax))) * 1.001;
    ts.mf_th.alpha = (float)(3.0 * 4.01 * u * L);   // x in fp32 is mu + w*sx: <= 2u relative
    ts.mf_th.beta = (float)(2.0 * ((ts.Dp + 4) * u * 1.01 + 4e-15));
    ts.mf_th.gamma = (float)(2.0 * 4.01 * u * u * L * L + 1e-30);
    ts.mf_th.inv_scale = (float)std::ldexp(1.0, -tt);
    // small-K scan (assign_small_kernel): each expanded score is an fp32 fma chain from n over
    // the D terms w_d * c''_d, with n and c'' rounded to fp32 once and w exact, so its error is
    // at most (D + 1) u (1 + u)^D (n + sum_d |w_d| |c''_d|) <= (D + 2) u S_row; two scores are
    // compared.  S_row <= 2^t (n_max + c2_max sum_d |w_d|), plus a 1e-11 relative floor for the
    // reference's own fp64 rounding (as e_conv above).
    const double sc = std::ldexp(1.0, tt);
    const double ks = 2.0 * (D + 2) * u * 1.01;
    ts.mf_th.e0 = (float)((ks * n_max + 1e-11 * s_bound) * sc * 1.0001);
    ts.mf_th.e1 = (float)(ks * c2_max * sc * 1.0001);
    ts.mf_th.mu = (float)t.mu;
    ts.mf_th.sx = (float)t.sx;
}

// The assignment pool grown to n buffers of N indices.  A view not yet set takes the buffer at its
// own position: the views set so far are a permutation of the buffers before it.
qvq_status ensure_apool(qvq_ctx *ctx, qvq_ctx::Training &ts, size_t n) {
    while (ts.apool.size() < n) {
        DevBuf<uint32_t> b;
        HIPCHK(b.alloc(ts.N));
        ts.apool.push_back(std::move(b));
    }
    uint32_t **views[4] = {&ts.d_A, &ts.d_A_alt, &ts.d_A3, &ts.d_A4};
    for (size_t i = 0; i < 4 && i < ts.apool.size(); i++)
        if (!*views[i]) *views[i] = ts.apool[i];
    return QVQ_OK;
}

// The resident set and everything sized by it dropped (the context then holds no training set).
void drop_training(qvq_ctx *ctx) {
    ctx->kh = {};
    ctx->ts = {};
    ctx->lv = {};
}

// Allocate the per-row buffers and upload the colour-space tables.
qvq_status alloc_training(qvq_ctx *ctx, uint64_t N, uint32_t D, int cs) {
    ctx->rf = qvq_ctx::RefineState();
    if (N == 0 || D == 0) return fail(ctx, QVQ_EINVAL, "empty training set");
    if (N >= (1ull << 32)) return fail(ctx, QVQ_EINVAL, "more than 2^32-1 rows per rank");
    const uint32_t Dp = (D + 3) & ~3u;
    if (Dp > 64) return fail(ctx, QVQ_EINVAL, "block dimension above 64 (3*w*h) is not supported");
    // the same shape again (repeated compresses of one image size): keep every buffer
    if (!ctx->ts.exact && ctx->ts.d_codes && ctx->ts.N == N && ctx->ts.D == D && ctx->ts.cs == cs) return QVQ_OK;
    drop_training(ctx);   // before the new set's allocations: peak memory is one set
    qvq_ctx::Training ts;   // moved into the context when it is complete
    if (!make_terms(cs, ts.terms)) return fail(ctx, QVQ_EUNSUPPORTED, "colour space has no exact byte sums");
    ts.N = N;
    ts.D = D;
    ts.Dp = Dp;
    ts.cs = cs;
    mfma_setup(ts);
    HIPCHK(ts.d_codes.alloc(N * Dp));
    qvq_status st = ensure_apool(ctx, ts, 1);
    if (st != QVQ_OK) return st;
    HIPCHK(ts.d_flags.alloc(N));
    HIPCHK(ts.d_ties.alloc(N));
    uint64_t plut[256];
    for (int b = 0; b < 256; b++) plut[b] = ((uint64_t)ts.terms.hi[b] << 32) | ts.terms.lo[b];
    HIPCHK(hipMemcpy(ctx->d_lut32, ts.terms.v32, sizeof(ts.terms.v32), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_w, ts.terms.w, sizeof(ts.terms.w), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_lut64, ts.terms.v64, sizeof(ts.terms.v64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_plut, plut, sizeof(plut), hipMemcpyHostToDevice));
    // the band of rows whose answer can depend on the centroids' last bits:
    // |c_kahan - c_exact| <= delta per component, so a distance moves by at most
    // 2 delta sqrt(D) sqrt(d) + D delta^2
    const double delta = cs == QVQ_CS_SCALED ? std::ldexp(1.0, -49) : 0.0;
    ts.tie_abs = 2 * delta * std::sqrt((double)D);
    ctx->ts = std::move(ts);
    return QVQ_OK;
}

qvq_status ensure_levels(qvq_ctx *ctx, uint32_t Kmax) {
    if (ctx->lv.Kcap >= Kmax) return QVQ_OK;
    ctx->lv = {};   // before the new buffers' allocations; a failure below leaves Kcap == 0
    qvq_ctx::Levels lv;
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t KD = (uint64_t)Kmax * D;
    const uint64_t Kp = pad32(Kmax);
    HIPCHK(lv.d_C64_cent.alloc(KD));
    HIPCHK(lv.d_C64_split.alloc(KD));
    HIPCHK(lv.d_C64_split_alt.alloc(KD));
    HIPCHK(lv.d_C32.alloc(Kp * Dp));
    if (D == MF_D) HIPCHK(lv.d_E32.alloc(Kp * 16));
    HIPCHK(lv.d_rows.alloc(Kp * cb_row_f16(D, Dp)));
    HIPCHK(lv.d_perm.alloc(Kp));
    HIPCHK(lv.d_tint.alloc(tint_bytes((uint32_t)Kp) / 4));
    // G per-CU slabs + two correction slabs (fused path: rows the recheck / kd-tree move, at
    // the new index (+) and at the search's provisional one (-))
    HIPCHK(lv.d_part.alloc((uint64_t)(ctx->G + 2) * KD));
    HIPCHK(lv.d_part_cnt.alloc((uint64_t)(ctx->G + 2) * Kmax));
    // two copies of the final sums: copy 1 takes the kd-tree ties' moves (kd_reduce_kernel) and
    // is cleared, over the level's region, by each fused search before the level's kd_reduce
    HIPCHK(lv.d_sums.alloc(2 * (2 * KD + Kmax)));
    HIPCHK(hipMemset(lv.d_sums, 0, lv.d_sums.bytes()));
    // two halves, each split rows | parent counts (host_cb_of)
    lv.cb_half = (KD + (uint64_t)Kmax / 2 + 1 + 7) / 8 * 8;
    HIPCHK(lv.h_cb.alloc(2 * lv.cb_half));
    lv.tree_cap = tree_bytes(Kmax, D);
    for (auto &h : lv.h_tree) HIPCHK(h.alloc(lv.tree_cap));
    HIPCHK(lv.d_tree.alloc(lv.tree_cap));
    {   // the device tree build's scratch (levels of up to KDB_MAXK code vectors)
        const uint32_t Kb = std::min<uint32_t>(Kmax, KDB_MAXK);
        if (plan_level(ctx, Kb).kd_device && kd_build_fits(Kb, D) && (uint64_t)Kmax * D >= KDB_MIN_KD) {
            HIPCHK(lv.d_kdb_vind.alloc(Kb));
            HIPCHK(lv.d_kdb_nodes.alloc(2ull * Kb));
            HIPCHK(lv.d_kdb_nbox.alloc(2ull * Kb * 2 * D));
            HIPCHK(lv.d_kdb_cbox.alloc(2ull * Kb * 2 * D));
            HIPCHK(lv.h_kdb.alloc(kdb_host_layout(Kb, D).total));
            std::memset(lv.h_kdb, 0, sizeof(KdbHeader));
            lv.kdb_cap = Kb;
            if (!ctx->kstream) HIPCHK(hipStreamCreateWithFlags(ctx->kstream.put(), hipStreamNonBlocking));
            if (!ctx->ev_kcb) HIPCHK(hipEventCreateWithFlags(ctx->ev_kcb.put(), hipEventDisableTiming));
            if (!ctx->ev_kdb) HIPCHK(hipEventCreateWithFlags(ctx->ev_kdb.put(), hipEventDisableTiming));
        }
    }
    lv.Kcap = Kmax;
    ctx->lv = std::move(lv);
    return QVQ_OK;
}

// What every finalize launch takes from the context: the terms, the centroids' and the tables'
// buffers and, with last_block, the end-of-kernel scratch, block counter and ready number.
FinArgs finalize_args(const qvq_ctx *ctx, uint32_t K, bool last_block) {
    const Terms &T = ctx->ts.terms;
    FinArgs f;
    f.K = K;
    f.D = ctx->ts.D;
    f.Dp = ctx->ts.Dp;
    f.R = T.R;
    f.bias = T.bias;
    f.scale = T.scale;
    f.mu = T.mu;
    f.sx = T.sx;
    f.t = ctx->ts.mf_t;
    f.C_cent = ctx->lv.d_C64_cent;
    f.C32 = ctx->lv.d_C32;
    f.rows = ctx->lv.d_rows;
    f.E32 = ctx->lv.d_E32;
    if (last_block) {
        f.dist_part = ctx->d_dist_part + 8;
        f.done = ctx->d_counters + FIN_DONE_COUNTER;
        f.ready = ctx->h_ready.dev();
    }
    return f;
}

// Copy 1 of d_sums sits one capacity-sized copy in, where no level's copy 0 reaches.
uint64_t sums_cap_stride(const qvq_ctx *ctx) { return 2 * (uint64_t)ctx->lv.Kcap * ctx->ts.D + ctx->lv.Kcap; }

// What run_level left of the level's sums, for reduce_level: a value that ends with the level
// (a level that is abandoned leaves nothing behind but, possibly, sums1_dirty).
struct LevelSums {
    // slabs of d_part / d_part_cnt to reduce (0: none, the sums are in d_sums), the last nsub subtracted
    uint32_t nslabs = 0, nsub = 0;
    // fused sums: slab G and its counts (the rows the recheck and the ties move at their new
    // index; slab G + 1, behind it, has them at the provisional one)
    uint64_t *xslab = nullptr;
    uint32_t *xcnt = nullptr;
    uint32_t copies = 1;    // 2: the ties' moves go to copy 1 of d_sums, which the finalize adds
    bool kd_pend = false;   // the kd-tree ties were left to the reduce (kd_reduce_kernel, over kd)
    KdView kd{};
    PubArgs pub;            // a tie-count publication left to the reduce
    bool upd = false;       // a separate sums pass ran between ev[slot][2] and [3]
};
// What reduce_level left in d_sums, for the finalize: the copies to add, and the gate of the
// copies past the first (the level's tie count), or null.
struct ReducedSums {
    uint32_t copies = 1;
    const unsigned *gate = nullptr;
};

// A writer of moves into copy 1 of d_sums (or of qvq_refine's changed total behind a level's
// sums, which lies in its range) says so first; the finalize that takes them lowers the flag.
void mark_sums1(qvq_ctx *ctx) { ctx->sums1_dirty = true; }
// Copy 1 of d_sums may hold moves that no finalize took (a call that stopped between the two):
// the sums cleared before they are used again.
qvq_status clear_dirty_sums(qvq_ctx *ctx) {
    if (ctx->sums1_dirty) {
        HIPCHK(hipMemsetAsync(ctx->lv.d_sums, 0, ctx->lv.d_sums.bytes(), ctx->stream));
        ctx->sums1_dirty = false;
    }
    return QVQ_OK;
}

// The sums side of a finalize: a level's reduced sums r (clear1: the finalize also clears copy 1
// after adding it, where no fused search of a later level does), or, r null, the mean sums at
// K = 1, which it leaves cleared for the next quantize.
void sums_args(const qvq_ctx *ctx, FinArgs &f, const ReducedSums *r, bool clear1) {
    f.sums = r ? ctx->lv.d_sums : ctx->d_mean;
    f.ncopy = r ? r->copies : MEAN_COPIES;
    f.cstride = r && r->copies > 1 ? sums_cap_stride(ctx) : 0;
    f.gate = r ? r->gate : nullptr;
    f.zero_sums = r ? clear1 && r->copies > 1 : true;
    f.zero_skip = r ? 1 : 0;
}
// The tables side: the search tables of the children * K code vectors the finalize writes to
// C_next (2: the split, 1: the same K), their host copy, and the tile order where the search
// that follows is pruned; the context then holds that K's order or none.
void tables_args(qvq_ctx *ctx, FinArgs &f, uint32_t children, double *C_next, double *host_cb, bool prune) {
    f.children = children;
    f.Kpad = pad32(children * f.K);
    f.C_next = C_next;
    f.host_cb = host_cb;
    if (prune) {
        f.perm = ctx->lv.d_perm;
        f.tint = ctx->lv.d_tint;
    }
    ctx->lv.perm_k = prune ? children * f.K : 0;
}
// Every finalize is launched here: one that adds copy 1 of the level's sums, or takes
// qvq_refine's changed total, has consumed what mark_sums1 announced.
qvq_status run_finalize(qvq_ctx *ctx, const FinArgs &f) {
    HIPCHK(launch_finalize(ctx->stream, f));
    if ((f.sums == ctx->lv.d_sums && f.ncopy > 1) || f.changed64) ctx->sums1_dirty = false;
    return QVQ_OK;
}

// Search tables for the K code vectors in d_C64_split (no tile order).
qvq_status run_prep(qvq_ctx *ctx, uint32_t K) {
    FinArgs f = finalize_args(ctx, K, false);
    f.C_src = ctx->lv.d_C64_split;
    tables_args(ctx, f, 1, nullptr, nullptr, false);
    return run_finalize(ctx, f);
}

// fp32 error-bound coefficients for the VALU search flag ("near-tie flags").
void valu_coeffs(const qvq_ctx *ctx, float &alpha, float &beta, float &gamma) {
    const double u = std::ldexp(1.0, -24);
    const double vmax = ctx->ts.terms.vmax;
    const double L = std::sqrt((double)ctx->ts.D) * (vmax + 1.2 * vmax) * 1.001;   // >= || |x| + |c| ||
    alpha = (float)(2.0 * 4.01 * u * L);
    beta = (float)(2.0 * ((ctx->ts.Dp + 4) * u * 1.01 + 4e-15));
    gamma = (float)(2.0 * 4.01 * u * u * L * L + 1e-30);
}

qvq_status wait_stream(qvq_ctx *ctx);

// Sum of count u64 (f64 = false) or double values at device pointer buf over the ranks, in
// place, on the context's stream: ncclAllReduce over xGMI, or -- the test-only host
// communicator of qvq_comm_init_host -- a copy to pinned memory, the caller's callback, and a
// copy back (the stream is drained around the callback).  No communicator: nothing to do.
qvq_status all_reduce(qvq_ctx *ctx, void *buf, uint64_t count, bool f64) {
    if (ctx->comm) {
        NCCLCHK(ncclAllReduce(buf, buf, count, f64 ? ncclDouble : ncclUint64, ncclSum, ctx->comm, ctx->stream));
        return QVQ_OK;
    }
    if (!ctx->host_ar) return QVQ_OK;
    HIPCHK(ctx->h_ar_stage.ensure(count * 8));
    qvq_status st;
    HIPCHK(hipMemcpyAsync(ctx->h_ar_stage, buf, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    const int rc = ctx->host_ar(ctx->h_ar_stage, count, f64 ? 1 : 0, ctx->host_ar_user);
    if (rc != 0) return fail(ctx, QVQ_ECOMM, "host all-reduce callback failed (" + std::to_string(rc) + ")");
    // stream-ordered: the next all-reduce's download (and callback) come after this upload
    HIPCHK(hipMemcpyAsync(buf, ctx->h_ar_stage, count * 8, hipMemcpyHostToDevice, ctx->stream));
    return QVQ_OK;
}

qvq_status all_reduce_sums(qvq_ctx *ctx, uint32_t K, uint64_t *sums = nullptr, uint32_t copies = 1) {
    if (!sums) sums = ctx->lv.d_sums;
    return all_reduce(ctx, sums, copies * (2 * (uint64_t)K * ctx->ts.D + K), false);
}

// Centroid sums under assignment d_A: nslabs slabs in d_part (for the reduce), or with the sort
// straight into d_sums (nslabs = 0).
qvq_status run_update_slabs(qvq_ctx *ctx, const LevelPlan &p, const uint32_t *d_A, uint32_t K, uint32_t &nslabs) {
    if (p.sorted_sums) {
        HIPCHK(ctx->ts.d_sortbuf.ensure(ctx->ts.N * 2));
        HIPCHK(launch_sorted_sums(ctx->stream, ctx->ts.Dp, ctx->G, ctx->ts.d_codes, ctx->ts.N, d_A, K, ctx->ts.D, ctx->d_plut,
                                  ctx->lv.d_part_cnt, reinterpret_cast<uint32_t *>(ctx->lv.d_part.get()), ctx->ts.d_sortbuf,
                                  ctx->ts.d_sortbuf + ctx->ts.N, ctx->lv.d_sums));
        nslabs = 0;
        return QVQ_OK;
    }
    HIPCHK(launch_update(ctx->stream, ctx->ts.Dp, ctx->G, ctx->ts.d_codes, ctx->ts.N, d_A, K, ctx->ts.D, ctx->d_plut, ctx->lv.d_part,
                         ctx->lv.d_part_cnt));
    nslabs = ctx->G;
    return QVQ_OK;
}

// ... and reduced into d_sums.
qvq_status run_update(qvq_ctx *ctx, const LevelPlan &p, const uint32_t *d_A, uint32_t K) {
    uint32_t nslabs = 0;
    qvq_status st = run_update_slabs(ctx, p, d_A, K, nslabs);
    if (st != QVQ_OK) return st;
    if (nslabs) HIPCHK(launch_reduce(ctx->stream, ctx->lv.d_part, ctx->lv.d_part_cnt, nslabs, 0, K, ctx->ts.D, ctx->lv.d_sums));
    return QVQ_OK;
}

// Reference-bit ties: the indices of the rows whose answer can depend on
// the centroids' last bits follow the reference's Kahan sums, on any rank count (several ranks:
// the chains run across the ranks, kahan_chained).  QVQ_KAHAN=0: the exact-sum codebook answers
// them (A/B).
bool kahan_mode(const qvq_ctx *ctx) {
    static const bool off = env_is("QVQ_KAHAN", "0");
    return !off && !ctx->ts.exact;
}
// The recheck's absolute tie band: only where a reference-bit step follows (kahan_mode)
double tie_band(const qvq_ctx *ctx) { return kahan_mode(ctx) ? ctx->ts.tie_abs : 0.0; }

// The Kahan outputs for Kc cells and a workspace for N rows, Kc cells and D components, each kept
// while it fits and otherwise rebuilt whole: released first, built in a local, moved in complete.
qvq_status ensure_kahan(qvq_ctx *ctx, uint32_t Kc) {
    qvq_ctx::Kahan &kh = ctx->kh;
    const uint64_t N = ctx->ts.N;
    const uint32_t D = ctx->ts.D;
    if (kh.cells.kcap < Kc) {
        kh.cells = {};
        qvq_ctx::Kahan::Cells c;
        HIPCHK(c.d_kc_cent.alloc((uint64_t)Kc * D));
        HIPCHK(c.d_kc_split.alloc(2ull * Kc * D));
        HIPCHK(c.d_kc_sel.alloc(Kc));
        HIPCHK(c.h_kc_sel.alloc(Kc));
        HIPCHK(c.h_kc_out.alloc(2ull * Kc * D));
        c.kcap = Kc;
        kh.cells = std::move(c);
    }
    if (kh.kw.n_cap == N && kh.kw.k_cap >= Kc && kh.kw.d_cap == D) return QVQ_OK;
    const uint32_t kcap = std::max(Kc, kh.kw.k_cap);
    kh.work = {};
    kh.kw = KahanWork();
    qvq_ctx::Kahan::Work b;
    uint64_t segs, blks;
    KahanWork::caps(N, kcap, segs, blks);
    HIPCHK(b.hist.alloc((uint64_t)KahanWork::sort_blocks(N) * kcap));
    HIPCHK(b.tot.alloc(kcap));
    for (auto *p : {&b.koff, &b.segoff, &b.blkoff}) HIPCHK(p->alloc((uint64_t)kcap + 1));
    HIPCHK(b.planes.alloc((uint64_t)D * KahanWork::plane_len(N)));
    HIPCHK(hipMemset(b.planes, 0, b.planes.bytes()));
    HIPCHK(b.meta.alloc((uint64_t)D * segs * KahanWork::meta_bytes()));
    HIPCHK(b.bsum.alloc((uint64_t)D * blks * 16));
    HIPCHK(b.bfn.alloc((uint64_t)D * blks * KahanWork::fn_bytes()));
    HIPCHK(b.sfn.alloc((uint64_t)D * segs * KahanWork::segfn_bytes()));
    HIPCHK(b.bfn8.alloc((uint64_t)D * blks * 8 * KahanWork::fn_bytes()));
    HIPCHK(b.stats.alloc(4));
    HIPCHK(hipMemset(b.stats, 0, b.stats.bytes()));
    {   // the byte table: SCALED values in units of 2^-60
        uint64_t kx[256];
        for (int i = 0; i < 256; i++) kx[i] = (uint64_t)std::ldexp(ctx->ts.terms.v64[i], 60);
        std::vector<uint8_t> tab(KahanWork::tab_bytes());
        KahanWork::make_tab(kx, tab.data());
        HIPCHK(b.tab.alloc(tab.size()));
        HIPCHK(hipMemcpy(b.tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
    KahanWork w;
    w.hist = b.hist, w.tot = b.tot, w.koff = b.koff, w.segoff = b.segoff, w.blkoff = b.blkoff;
    w.planes = b.planes, w.meta = b.meta, w.bsum = b.bsum, w.bfn = b.bfn, w.sfn = b.sfn, w.bfn8 = b.bfn8;
    w.tab = b.tab, w.stats = b.stats;
    w.n_one = (uint32_t)N;
    w.seg_cap = segs;
    w.blk_cap = blks;
    w.n_cap = N;
    w.k_cap = kcap;
    w.d_cap = D;
    kh.work = std::move(b);
    kh.kw = w;
    return QVQ_OK;
}


// Sum over the ranks of n small u64 values (host, in place) on the context's stream, waiting for
// the result: the ranks' decisions at the end of qvq_lbg, so that every rank takes the same
// branch.  One rank: nothing to do.
qvq_status vote(qvq_ctx *ctx, uint64_t *vals, uint64_t n) {
    if (ctx->nranks <= 1 || (!ctx->comm && !ctx->host_ar) || n == 0) return QVQ_OK;
    HIPCHK(ctx->d_vote.ensure(n));
    HIPCHK(ctx->h_vote.ensure(n));
    std::memcpy(ctx->h_vote, vals, n * 8);
    HIPCHK(hipMemcpyAsync(ctx->d_vote, ctx->h_vote, n * 8, hipMemcpyHostToDevice, ctx->stream));
    qvq_status st = all_reduce(ctx, ctx->d_vote, n, false);
    if (st != QVQ_OK) return st;
    HIPCHK(hipMemcpyAsync(ctx->h_vote, ctx->d_vote, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    std::memcpy(vals, ctx->h_vote, n * 8);
    return QVQ_OK;
}

// The reference's Kahan centroids (and their split) of S cells when the rows are split over the
// ranks, each rank holding a contiguous range of the global rows, ranks in row order (DESIGN.md
// 5; src/Quantizer.cpp:59-70 sums each cell's rows in ascending global order, so a chain runs
// across the ranks).  A: this rank's rows' cells among K_in (nullptr: the mean, K_in = S = 1);
// sel: the device slot map of launch_kahan_centroids (nullptr: every cell, S = K_in).  Every
// rank calls it with the same cells and gets the same centroids in d_kc_cent [S][D] and, with
// want_split, their split in d_kc_split [2S][D] (device; ensure_kahan sizes both):
//   1. each rank sorts its rows of the cells and sums each chain exactly (its totals and row
//      counts into its slice of an all-gather, one collective): every chain's exact prefix at
//      each rank's first row;
//   2. each rank builds its segment functions at those global prefixes;
//   3. the chains pass from rank to rank: rank q advances the reference's state (sum, c) over
//      its rows and an all-reduce, the others contributing zeros, hands it on (nranks small
//      collectives);
//   4. C = sum * fl(1/n), n the cell's rows over every rank.
// splits (qvq_update_kahan_split, tests): this context's rows as virtual ranks cut at the given
// offsets, run one after another on the device (no collective).
qvq_status kahan_chained(qvq_ctx *ctx, const uint32_t *A, uint32_t K_in, const uint32_t *sel, uint32_t S,
                         bool want_split, const std::vector<uint64_t> *splits = nullptr) {
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const bool virt = splits != nullptr;
    const uint32_t R = virt ? (uint32_t)splits->size() - 1 : (uint32_t)ctx->nranks;
    const uint32_t rank = virt ? 0u : (uint32_t)ctx->rank;
    const uint32_t Ks = sel ? S : K_in;   // the sort's keys: slots, or cells
    if (!A && (K_in != 1 || S != 1 || sel)) return fail(ctx, QVQ_EINVAL, "kahan_chained: the mean is one cell");
    qvq_status st = ensure_kahan(ctx, std::max(K_in, S));   // (may reallocate the outputs below)
    if (st != QVQ_OK) return st;
    double *C_out = ctx->kh.cells.d_kc_cent, *split_out = want_split ? ctx->kh.cells.d_kc_split : nullptr;
    const uint64_t gcount = 2ull * R * S * D + (uint64_t)R * S, scount = 2ull * S * D;
    HIPCHK(ctx->kh.d_kc_chain.ensure(gcount + scount));
    uint64_t *gather = ctx->kh.d_kc_chain, *state = gather + gcount;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemsetAsync(gather, 0, (gcount + scount) * 8, s));
    const KahanWork &w = ctx->kh.kw;
    if (virt) {
        for (uint32_t v = 0; v < R; v++) {
            const uint64_t off = (*splits)[v], n = (*splits)[v + 1] - off;
            if (!n) continue;
            const uint8_t *codes = ctx->ts.d_codes + off * Dp;
            const uint32_t *Av = A ? A + off : nullptr;
            HIPCHK(launch_kahan_chain_local(s, w, codes, Dp, D, n, Av, Ks, sel, K_in, gather, v, R));
            HIPCHK(launch_kahan_chain_build(s, w, D, n, Ks, gather, v));
            HIPCHK(launch_kahan_chain_eval(s, w, D, n, Ks, state, gather, v));
        }
    } else {
        HIPCHK(launch_kahan_chain_local(s, w, ctx->ts.d_codes, Dp, D, ctx->ts.N, A, Ks, sel, K_in, gather, rank, R));
        if (R > 1 && (st = all_reduce(ctx, gather, gcount, false)) != QVQ_OK) return st;
        HIPCHK(launch_kahan_chain_build(s, w, D, ctx->ts.N, Ks, gather, rank));
        for (uint32_t q = 0; q < R; q++) {
            if (q == rank) HIPCHK(launch_kahan_chain_eval(s, w, D, ctx->ts.N, Ks, state, gather, rank));
            else HIPCHK(hipMemsetAsync(state, 0, scount * 8, s));
            if (R > 1 && (st = all_reduce(ctx, state, scount, false)) != QVQ_OK) return st;
        }
    }
    HIPCHK(launch_kahan_chain_finish(s, D, Ks, state, gather, R, C_out, split_out));
    return QVQ_OK;
}

// Build the reference kd-tree over the host copy hC of the K code vectors being searched
// into tree image buffer buf (pinned host memory, DMA-copied to d_tree for kd_resolve_kernel).  An empty
// view means host resolution (tree too deep/large for the kernel's LDS, or QVQ_KDTREE=host).

// Level L's split codebook as the finalize of level L - 1 publishes it (host / device view).
// Double-buffered by level parity: the synchronous Kahan levels build a level's tree on the
// worker from this copy while the level's own finalize already publishes the next level's
// codebook (one buffer: a worker late by more than the level's search read a mix of the two,
// the r05i-r05m intermittent mismatches on palette images).
// QVQ_CB_SINGLE=1 (tests only): the one buffer of before the fix, which with
// QVQ_TREE_JOB_DELAY_MS makes the race deterministic (tests/test_gpu_kahan.py).
uint32_t cb_half_of(uint32_t level) {
    static const bool single = env_is("QVQ_CB_SINGLE", "1");
    return single ? 0u : (level & 1);
}
double *host_cb_of(const qvq_ctx *ctx, uint32_t level) { return ctx->lv.h_cb + (uint64_t)cb_half_of(level) * ctx->lv.cb_half; }
double *dev_cb_of(const qvq_ctx *ctx, uint32_t level) { return ctx->lv.h_cb.dev() + (uint64_t)cb_half_of(level) * ctx->lv.cb_half; }

// The host part: the tree (ctx->tree over ctx->cb_local) and its flattened image in h_tree[buf];
// v.bytes = 0 when there is no device image (too large, or too deep for the kernel's LDS).
// No HIP call: the tree worker runs it.
void build_tree_host(qvq_ctx *ctx, const double *hC, uint32_t K, int buf, KdView &v,
                     const std::atomic<bool> *cancel = nullptr) {
    v = KdView{};
    // the build reads the codebook many times; mapped memory the GPU just wrote is read
    // once, sequentially, into ordinary memory first
    ctx->cb_local.assign(hC, hC + (size_t)K * ctx->ts.D);
    if ((hC == host_cb_of(ctx, 0) || hC == host_cb_of(ctx, 1)) && K >= 2) {   // a finalize's split: the parent counts follow it
        const uint32_t *cnt = reinterpret_cast<const uint32_t *>(hC + (size_t)K * ctx->ts.D);
        ctx->cnt_local.assign(cnt, cnt + K / 2);
    } else {
        ctx->cnt_local.clear();
    }
    ctx->htrace.mark("K" + std::to_string(K) + " codebook copied");
    ctx->tree.reset(new RefKDTree(ctx->cb_local.data(), K, (int)ctx->ts.D, cancel));
    ctx->htrace.mark("K" + std::to_string(K) + " tree structure");
    const RefKDTree &tree = *ctx->tree;
    if (tree.cancelled()) return;
    const uint32_t D = ctx->ts.D;
    const size_t nn = tree.num_nodes();
    KdView t;
    t.depth = tree.depth();
    t.n_nodes = (uint32_t)nn;
    const uint64_t bytes = 16ull * D + nn * sizeof(KdNodeDev) + 4ull * K;
    if (bytes > ctx->lv.tree_cap) return;
    t.bytes = (uint32_t)bytes;
    if (!kd_resolve_fits(t, K)) return;
    double *lo = reinterpret_cast<double *>(ctx->lv.h_tree[buf].get()), *hi = lo + D;
    KdNodeDev *nodes = reinterpret_cast<KdNodeDev *>(hi + D);
    uint32_t *vind = reinterpret_cast<uint32_t *>(nodes + nn);
    tree.flatten(nodes, vind, lo, hi);
    v = t;
}

// The device view of image buf (v from build_tree_host).  Every kd_resolve workgroup stages the
// image.  Big images (C4: 150+ KB) go to device memory with one DMA first (mapped reads from 16
// workgroups cost up to ~70 us); small ones are read in place (the DMA itself costs ~5 us of
// stream time per level).
void tree_view(qvq_ctx *ctx, int buf, KdView &v) {
    if (!v.bytes) {
        v = KdView{};
        return;
    }
    const uint32_t D = ctx->ts.D;
    const double *dlo = reinterpret_cast<const double *>(ctx->lv.h_tree[buf].dev());
    constexpr uint64_t dma_min = 32768;
    if (v.bytes > dma_min) {
        if (hipMemcpyAsync(ctx->lv.d_tree, ctx->lv.h_tree[buf], v.bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            v = KdView{};
            return;
        }
        dlo = reinterpret_cast<const double *>(ctx->lv.d_tree.get());
    }
    v.lo = dlo;
    v.hi = dlo + D;
    v.nodes = reinterpret_cast<const KdNodeDev *>(dlo + 2 * D);
    v.vind = reinterpret_cast<const uint32_t *>(v.nodes + v.n_nodes);
}

void build_tree(qvq_ctx *ctx, const LevelPlan &p, const double *hC, uint32_t K, int buf, KdView &kd) {
    kd = KdView{};
    ctx->tree_kd = KdView{};
    if (p.kd_host) return;
    build_tree_host(ctx, hC, K, buf, kd);
    tree_view(ctx, buf, kd);
    ctx->tree_kd = kd;
}

CommState probe_comm(qvq_ctx *ctx, std::string &msg);
qvq_status wait_failed(qvq_ctx *ctx, qvq_status st);

// The device build of a level's tree (k_kdbuild.hip; plan_level: QVQ_KDTREE=device, 48-D levels
// from K = 512 up to KDB_MAXK; bit-identical to the host build, tests/test_gpu_kdbuild.py),
// enqueued over the K code vectors in d_C64_split on kstream, after the work already on the
// context's stream (the finalize that wrote them); the search then runs beside it.
qvq_status start_device_tree(qvq_ctx *ctx, uint32_t K) {
    HIPCHK(hipEventRecord(ctx->ev_kcb, ctx->stream));
    HIPCHK(hipStreamWaitEvent(ctx->kstream, ctx->ev_kcb, 0));
    HIPCHK(launch_kd_build(ctx->kstream, ctx->lv.d_C64_split, K, ctx->ts.D, ctx->lv.d_kdb_vind, ctx->lv.d_kdb_nodes,
                           ctx->lv.d_kdb_nbox, ctx->lv.d_kdb_cbox, ctx->lv.d_tree, ctx->lv.h_kdb.dev(), ++ctx->kdb_seq));
    HIPCHK(hipEventRecord(ctx->ev_kdb, ctx->kstream));
    return QVQ_OK;
}

// The device build's tree for the level: waits (bounded) for its image, makes the context's
// stream wait for the build (d_C64_split is rewritten by the level's finalize), and imports it as
// ctx->tree over ctx->cb_local (which the caller filled) with its device view in kd.  false: the
// build failed (the caller builds on the host).
qvq_status finish_device_tree(qvq_ctx *ctx, uint32_t K, KdView &kd, bool &ok) {
    ok = false;
    kd = KdView{};
    const KdbHeader *h = reinterpret_cast<const KdbHeader *>(ctx->lv.h_kdb.get());
    std::string err;
    const qvq_status st = wait_until(
        [&] { return *reinterpret_cast<const volatile uint64_t *>(&h->seq) >= ctx->kdb_seq; },
        [&](std::string &m) {
            const hipError_t q = hipStreamQuery(ctx->kstream);
            if (q == hipSuccess) return StreamState::Drained;
            if (q == hipErrorNotReady) return StreamState::Running;
            m = hipGetErrorString(q);
            return StreamState::Failed;
        },
        [&](std::string &m) { return probe_comm(ctx, m); }, ctx->timeout_s, err);
    if (st != QVQ_OK) return wait_failed(ctx, fail(ctx, st, "device kd-tree build: " + err));
    std::atomic_thread_fence(std::memory_order_acquire);
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_kdb, 0));
    if (h->status != 1) return QVQ_OK;
    ctx->tree.reset(new RefKDTree(ctx->cb_local.data(), K, (int)ctx->ts.D, ctx->lv.h_kdb));
    KdView t;
    t.depth = (int)h->depth;
    t.n_nodes = h->n_nodes;
    const uint64_t bytes = 16ull * ctx->ts.D + (uint64_t)h->n_nodes * sizeof(KdNodeDev) + 4ull * K;
    ok = true;
    if (bytes > ctx->lv.tree_cap) return QVQ_OK;
    t.bytes = (uint32_t)bytes;
    if (!kd_resolve_fits(t, K)) return QVQ_OK;
    const double *dlo = reinterpret_cast<const double *>(ctx->lv.d_tree.get());
    t.lo = dlo;
    t.hi = dlo + ctx->ts.D;
    t.nodes = reinterpret_cast<const KdNodeDev *>(dlo + 2 * ctx->ts.D);
    t.vind = reinterpret_cast<const uint32_t *>(t.nodes + t.n_nodes);
    kd = t;
    return QVQ_OK;
}

// A deferred-tie level (qvq_lbg's Kahan path) needs its tree only when it has ties, which the
// host learns after the search: the worker awaits the codebook's publication and builds the
// tree while this thread enqueues the rest of the level; join_tree_job waits for it (ties)
// or cancels it (none).
void post_job(qvq_ctx *ctx, std::function<void()> job, qvq_ctx::Worker *wk = nullptr) {
    qvq_ctx::Worker &w = wk ? *wk : ctx->worker;
    if (!w.th.joinable()) {
        w.th = std::thread([&w] {
            std::unique_lock<std::mutex> lk(w.m);
            for (;;) {
                w.cv.wait(lk, [&w] { return w.stop || !w.q.empty(); });
                if (w.stop && w.q.empty()) return;   // (queued frees still run)
                std::function<void()> job = std::move(w.q.front());
                w.q.pop_front();
                lk.unlock();
                job();
                w.pending.fetch_sub(1, std::memory_order_release);
                lk.lock();
            }
        });
        if (ctx->place_ok) pthread_setaffinity_np(w.th.native_handle(), sizeof(cpu_set_t), &ctx->place);
    }
    w.pending.fetch_add(1, std::memory_order_relaxed);
    {
        std::lock_guard<std::mutex> g(w.m);
        w.q.push_back(std::move(job));
    }
    w.cv.notify_one();
}

bool join_tree_job(qvq_ctx *ctx, bool cancel) {
    if (!ctx->tree_job) return false;
    if (cancel) ctx->tree_cancel.store(true);
    while (ctx->worker.pending.load(std::memory_order_acquire)) std::this_thread::yield();
    ctx->tree_job = false;
    if (!ctx->job_ok) {
        ctx->tree.reset();
        ctx->tree_kd = KdView{};
        return false;
    }
    KdView v = ctx->job_kd;
    tree_view(ctx, ctx->job_buf, v);
    ctx->tree_kd = v;
    return true;
}

void start_tree_job(qvq_ctx *ctx, const LevelPlan &p, const double *hC, uint32_t K, int buf, uint64_t wait_seq) {
    join_tree_job(ctx, true);
    if (p.kd_host) return;
    ctx->tree_cancel.store(false);
    ctx->tree_job = true;
    ctx->job_ok = false;
    ctx->job_buf = buf;
    ctx->tree_kd = KdView{};
    const int slot = (int)__builtin_ctz(K) - 1;
    post_job(ctx, [ctx, hC, K, buf, wait_seq, slot] {
        const auto t0 = std::chrono::steady_clock::now();
        volatile uint64_t *flag = ctx->h_ready;
        while (wait_seq && *flag < wait_seq) {   // the codebook's publication (bounded by cancel)
            if (ctx->tree_cancel.load(std::memory_order_relaxed)) return;
            cpu_relax();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        // QVQ_TREE_JOB_DELAY_MS (tests only): a worker late past the level's own finalize, the
        // interleaving of the r05m race (the finalize publishes the next level's codebook)
        static const int delay_ms = std::getenv("QVQ_TREE_JOB_DELAY_MS") ? std::atoi(std::getenv("QVQ_TREE_JOB_DELAY_MS")) : 0;
        if (delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(delay_ms));
        const auto t1 = std::chrono::steady_clock::now();
        build_tree_host(ctx, hC, K, buf, ctx->job_kd, &ctx->tree_cancel);
        ctx->job_ok = !ctx->tree->cancelled();
        ctx->tm.wait_ms[slot] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        ctx->tm.tree_ms[slot] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    });
}

// Copy between a caller's host buffer and device memory at DMA speed: the host range is pinned
// in place for the copy (hipHostRegister; a pageable hipMemcpy goes through bounce buffers at a
// fraction of PCIe bandwidth: the 50 MB C3 raster took ~3 ms), with a plain copy as the fallback
// (already pinned memory, or registration refused).
// Synchronous on the context's stream.
hipError_t host_copy(qvq_ctx *ctx, void *dst, const void *src, uint64_t bytes, hipMemcpyKind kind) {
    void *host = const_cast<void *>(kind == hipMemcpyHostToDevice ? src : dst);
    const bool reg = bytes >= (1u << 20) && hipHostRegister(host, bytes, hipHostRegisterDefault) == hipSuccess;
    if (!reg) (void)hipGetLastError();
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (reg) (void)hipHostUnregister(host);
    return e;
}

// Probes for wait_until (wait.hpp): the stream's state, and the communicator's asynchronous
// error state (RCCL reports a peer's failure there while our collective is stuck).
StreamState probe_stream(qvq_ctx *ctx, std::string &msg) {
    const hipError_t q = hipStreamQuery(ctx->stream);
    if (q == hipSuccess) return StreamState::Drained;
    if (q == hipErrorNotReady) return StreamState::Running;
    msg = hipGetErrorString(q);
    return StreamState::Failed;
}
CommState probe_comm(qvq_ctx *ctx, std::string &msg) {
    if (!ctx->comm) return CommState::None;
    ncclResult_t ae = ncclSuccess;
    const ncclResult_t r = ncclCommGetAsyncError(ctx->comm, &ae);
    if (r != ncclSuccess) ae = r;
    if (ae == ncclSuccess || ae == ncclInProgress) return CommState::Healthy;
    msg = ncclGetErrorString(ae);
    return CommState::Failed;
}
// A failed or timed-out wait: a communicator is aborted (which also releases the stream from
// a stuck RCCL kernel) and the context runs single-rank until the next qvq_comm_init.  Then
// the stream gets one more bounded chance to drain; if it does not (a timeout without a
// communicator, a kernel still running), the context is poisoned: work that may still write
// the context's scratch or copy into caller memory is queued, so every later call but
// qvq_destroy returns QVQ_ESTATE.
qvq_status wait_failed(qvq_ctx *ctx, qvq_status st) {
    if (st == QVQ_ECOMM && ctx->comm) {
        (void)ncclCommAbort(ctx->comm);
        ctx->comm = nullptr;
        ctx->nranks = 1;
        ctx->rank = 0;
    }
    using clock = std::chrono::steady_clock;
    // after an abort the RCCL kernels exit: give the stream 2 s to drain; a timeout without a
    // communicator means a long or stuck kernel: one query
    const auto until = clock::now() + std::chrono::milliseconds(st == QVQ_ECOMM ? 2000 : 0);
    hipError_t q = hipStreamQuery(ctx->stream);
    while (q == hipErrorNotReady && clock::now() < until) q = hipStreamQuery(ctx->stream);
    if (q != hipSuccess) {
        ctx->poisoned = true;
        ctx->err += " (context poisoned: destroy it)";
    }
    return st;
}

// Wait until the stream has published seq in a mapped flag (the ready number of finalize's
// codebook in h_ready, or copy_out's completion).  Bounded: a failed or drained stream, a
// communicator error, or ctx->timeout_s without progress end the wait with a status.
qvq_status wait_flag(qvq_ctx *ctx, volatile uint64_t *flag, uint64_t seq) {
    std::string err;
    const qvq_status st = wait_until([&] { return *flag >= seq; },
                                     [&](std::string &m) { return probe_stream(ctx, m); },
                                     [&](std::string &m) { return probe_comm(ctx, m); }, ctx->timeout_s, err);
    if (st != QVQ_OK) return wait_failed(ctx, fail(ctx, st, err));
    std::atomic_thread_fence(std::memory_order_acquire);
    return QVQ_OK;
}
// Wait for everything enqueued on the stream so far (an event, polled with the same bounds).
qvq_status wait_stream(qvq_ctx *ctx) {
    HIPCHK(hipEventRecord(ctx->ev_sync, ctx->stream));
    std::string err;
    hipError_t eq = hipSuccess;
    const qvq_status st = wait_until(
        [&] {
            eq = hipEventQuery(ctx->ev_sync);
            return eq != hipErrorNotReady;
        },
        [&](std::string &m) { return probe_stream(ctx, m); }, [&](std::string &m) { return probe_comm(ctx, m); },
        ctx->timeout_s, err);
    if (st != QVQ_OK) return wait_failed(ctx, fail(ctx, st, err));
    if (eq != hipSuccess) return fail(ctx, QVQ_EDEVICE, std::string("stream: ") + hipGetErrorString(eq));
    return QVQ_OK;
}
qvq_status wait_codebook(qvq_ctx *ctx, uint64_t seq) { return wait_flag(ctx, ctx->h_ready, seq); }

// Tie rows listed by the recheck when no device tree was available: answer them with the
// host tree over hC and write A; with xslab / xcnt (LevelSums) their terms move from the search's
// provisional index to the answer, with xsums within finished sums (launch_fix_rows).  Synchronous.
qvq_status resolve_host_ties(qvq_ctx *ctx, const double *hC, uint32_t K, uint32_t nt, uint64_t *xslab, uint32_t *xcnt,
                             uint64_t *xsums) {
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t need = (uint64_t)nt * (8 + Dp);
    HIPCHK(ctx->d_scatter.ensure(need / 4));
    uint32_t *d_rows = ctx->d_scatter, *d_vals = ctx->d_scatter + nt;
    uint8_t *d_gath = reinterpret_cast<uint8_t *>(ctx->d_scatter + 2 * (uint64_t)nt);
    std::vector<uint32_t> rows(nt), vals(nt);
    std::vector<uint8_t> code((uint64_t)nt * Dp);
    HIPCHK(launch_gather_codes(ctx->stream, ctx->ts.d_codes, Dp, ctx->ts.d_ties, nt, d_gath));
    HIPCHK(hipMemcpyAsync(rows.data(), ctx->ts.d_ties, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(code.data(), d_gath, code.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<double> q(D);
    RefKDTree tree(hC, K, (int)D);
    for (uint32_t i = 0; i < nt; i++) {
        for (uint32_t d = 0; d < D; d++) q[d] = ctx->ts.terms.v64[code[(uint64_t)i * Dp + d]];
        vals[i] = tree.nearest(q.data());
    }
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_vals, vals.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_fix_rows(ctx->stream, ctx->ts.d_codes, Dp, D, ctx->ts.d_A, d_rows, d_vals, nt, K, xslab, xcnt,
                           ctx->d_plut, xsums));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the host vectors must outlive the copies
    return QVQ_OK;
}

// One rank, fused sums: the kd-tree ties go with the reduce (kd_reduce_kernel: one launch fewer
// per level).
bool kd_merge(const qvq_ctx *ctx) { return !ctx->comm && !ctx->host_ar; }

// One level's assignment of every row against the split codebook (d_C64_split, host copy
// hC, search tables in d_C32/d_rows), K code vectors.  wait_seq != 0: hC is published by a
// finalize still in flight.  In: the level's plan p (plan_level of this K) and the call's own
// facts -- sums_out, defer_ties (the ties wait for the caller's reference-bit step), whether a
// communicator is joined (kd_merge) and whether the context holds this K's tile order (perm_k),
// which meet the plan in the first lines below.  Out: with sums_out, ls describes where the
// exact centroid sums of the final assignment are, for reduce_level (fused: the search's G slabs
// with every row at its provisional index and the two correction slabs; otherwise the sums
// pass's G slabs, or the sums themselves, reduced already).
qvq_status run_level(qvq_ctx *ctx, const LevelPlan &p, uint32_t K, int slot, bool sums_out, const double *hC,
                     uint64_t wait_seq, bool defer_ties, LevelSums &ls) {
    ls = LevelSums();
    const bool fused = sums_out && p.fusable;
    // one rank, sums from a separate pass: that pass (and its reduce) runs before the tree is
    // built -- it overlaps the host build instead of waiting behind it -- and the ties' moves are
    // then applied to the finished sums (move_row_sums)
    const bool early_upd = sums_out && !fused && (kd_merge(ctx) || defer_ties);
    // the order the finalize before this level left: valid for the search and the recheck
    const bool pruned = ctx->lv.perm_k == K;
    // the level's kd-tree on the device, beside the search (every CU holds a search workgroup
    // and room for the build's)
    const bool devtree = !defer_ties && p.kd_device && p.tree_shape && ctx->lv.kdb_cap >= K && !ctx->ts.exact;
    uint64_t *sums1 = early_upd ? ctx->lv.d_sums : nullptr;
    if (fused) {
        ls.xslab = ctx->lv.d_part + (uint64_t)ctx->G * K * ctx->ts.D;
        ls.xcnt = ctx->lv.d_part_cnt + (uint64_t)ctx->G * K;
        ls.nslabs = ctx->G + 2;
        ls.nsub = 1;
    } else if (sums_out) {
        ls.nslabs = ctx->G;
    }
    const uint32_t *perm = pruned ? ctx->lv.d_perm : nullptr;
    const int32_t *tint = pruned ? ctx->lv.d_tint : nullptr;
    unsigned *cnt = ctx->d_counters + 2 * slot;
    // HIP events around the search (each record costs a few us of GPU idle): every level,
    // one level, or none (qvq_set_timing)
    const bool timing = ctx->timing_level == -1 || ctx->timing_level == slot;
    qvq_status st;
    if (devtree && (st = start_device_tree(ctx, K)) != QVQ_OK) return st;
    if (timing) HIPCHK(hipEventRecord(ctx->ev[slot][0], ctx->stream));
    if (p.mfma()) {
        // one rank, fused sums: the search clears copy 1 of the final sums (the kd ties' moves,
        // added by the previous level's finalize), covering every smaller level's layout
        const bool clear1 = fused && kd_merge(ctx);
        HIPCHK(launch_assign_mfma(ctx->stream, ctx->num_cu, fused, ctx->ts.d_codes, ctx->ts.N, ctx->lv.d_rows, ctx->lv.d_E32, K,
                                  ctx->lv.d_C32, ctx->d_plut, ctx->ts.mf_th, ctx->ts.d_A, ctx->ts.d_flags, &cnt[0],
                                  ctx->lv.d_part, ctx->lv.d_part_cnt, perm, tint,
                                  clear1 ? ctx->lv.d_sums + sums_cap_stride(ctx) : nullptr,
                                  clear1 ? (uint32_t)(2 * (uint64_t)K * ctx->ts.D + K) : 0u));
    } else if (p.search == QVQ_PLAN_SEARCH_WIDE) {
        HIPCHK(launch_assign_wide(ctx->stream, ctx->num_cu, ctx->ts.Dp, ctx->ts.D, ctx->ts.d_codes, ctx->ts.N, ctx->lv.d_rows, K,
                                  ctx->lv.d_C32, ctx->ts.mf_th, ctx->ts.d_A, ctx->ts.d_flags, &cnt[0], perm, tint,
                                  std::max<uint32_t>(1, (ctx->col_blocks + 32) / 64), ctx->d_counters + SCHED_COUNTERS));
    } else {
        float alpha, beta, gamma;
        valu_coeffs(ctx, alpha, beta, gamma);
        HIPCHK(launch_assign_valu(ctx->stream, ctx->num_cu, ctx->ts.Dp, ctx->ts.d_codes, ctx->ts.N, ctx->lv.d_C32, K,
                                  ctx->d_lut32, alpha, beta, gamma, ctx->ts.d_A, ctx->ts.d_flags, &cnt[0]));
    }
    if (timing) HIPCHK(hipEventRecord(ctx->ev[slot][1], ctx->stream));
    if (p.recheck == QVQ_PLAN_RECHECK_MF32) {
        HIPCHK(launch_recheck_mf32(ctx->stream, ctx->num_cu, ctx->ts.d_codes, ctx->ts.d_flags, &cnt[0], ctx->lv.d_rows,
                                   ctx->lv.d_C64_split, K, ctx->d_lut64, ctx->ts.mf_th, 1e-12, tie_band(ctx), ctx->ts.d_A, ctx->ts.d_ties,
                                   &cnt[1], ls.xslab, ls.xcnt, ctx->d_plut));
    } else {
        float alpha, beta, gamma;
        valu_coeffs(ctx, alpha, beta, gamma);
        HIPCHK(launch_recheck(ctx->stream, ctx->num_cu, ctx->ts.d_codes, ctx->ts.Dp, ctx->ts.D, ctx->ts.d_flags, &cnt[0],
                              ctx->lv.d_C64_split, ctx->lv.d_C32, K, ctx->d_lut64, alpha, beta, gamma, 1e-12, tie_band(ctx), ctx->ts.d_A,
                              ctx->ts.d_ties, &cnt[1], ls.xslab, ls.xcnt, ctx->d_plut, perm, tint,
                              (float)((double)ctx->ts.D / (ctx->ts.terms.sx * ctx->ts.terms.sx))));
    }
    if (defer_ties) {   // the level's tie count to the host, before the rest of the level runs
        ctx->pub_seq++;
        if (fused) {   // published by the slab reduce that follows (reduce_level): no launch of its own
            ls.pub.cnt = &cnt[1];
            ls.pub.dst = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->h_ready.dev()) + 16);
            ls.pub.flag = ctx->h_ready.dev() + 1;
            ls.pub.seq = ctx->pub_seq;
        } else {
            HIPCHK(launch_copy_out(ctx->stream, &cnt[1], reinterpret_cast<uint8_t *>(ctx->h_ready.dev()) + 16, 4, nullptr,
                                   nullptr, 0, nullptr, nullptr, 0, ctx->h_ready.dev() + 1, ctx->pub_seq,
                                   ctx->d_counters + COPY_DONE_COUNTER));
        }
    }
    if (early_upd) {
        HIPCHK(hipEventRecord(ctx->ev[slot][2], ctx->stream));
        if ((st = run_update(ctx, p, ctx->ts.d_A, K)) != QVQ_OK) return st;
        ls.nslabs = 0;   // reduced already
        HIPCHK(hipEventRecord(ctx->ev[slot][3], ctx->stream));
    }
    if (defer_ties) {   // qvq_lbg answers the ties after the finalize, if there are any (tree on the worker)
        start_tree_job(ctx, p, hC, K, slot & 1, wait_seq);
        return QVQ_OK;
    }
    // the tree build overlaps the search just enqueued
    const auto tw0 = std::chrono::steady_clock::now();
    if (wait_seq && (st = wait_codebook(ctx, wait_seq)) != QVQ_OK) return st;
    const auto tw1 = std::chrono::steady_clock::now();
    ctx->htrace.mark("K" + std::to_string(K) + " codebook seen, tree build");
    KdView kd;
    bool dev_ok = false;
    if (devtree) {   // the host copies of the codebook and parent counts, then the device's tree
        ctx->cb_local.assign(hC, hC + (size_t)K * ctx->ts.D);
        if ((hC == host_cb_of(ctx, 0) || hC == host_cb_of(ctx, 1)) && K >= 2) {
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(hC + (size_t)K * ctx->ts.D);
            ctx->cnt_local.assign(pc, pc + K / 2);
        } else {
            ctx->cnt_local.clear();
        }
        if ((st = finish_device_tree(ctx, K, kd, dev_ok)) != QVQ_OK) return st;
        ctx->tree_kd = kd;
    }
    if (!dev_ok) build_tree(ctx, p, hC, K, slot & 1, kd);
    ctx->htrace.mark("K" + std::to_string(K) + (dev_ok ? " device tree in" : " tree built"));
    ctx->tm.wait_ms[slot] = std::chrono::duration<double, std::milli>(tw1 - tw0).count();
    ctx->tm.tree_ms[slot] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count();
    if (kd.depth > 0 && fused && kd_merge(ctx) && kd_reduce_fits(kd, K)) {
        ls.kd_pend = true;   // with the reduce (reduce_level)
        ls.kd = kd;
        ls.copies = 2;
    } else if (kd.depth > 0) {
        HIPCHK(launch_kd_resolve(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, ctx->ts.D, ctx->ts.d_ties, &cnt[1], ctx->lv.d_C64_split,
                                 K, ctx->d_lut64, kd, ctx->ts.d_A, ls.xslab, ls.xcnt, ctx->d_plut, sums1));
    } else {   // ties answered on the host
        unsigned nt = 0;
        HIPCHK(hipMemcpyAsync(&nt, &cnt[1], sizeof(nt), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (nt && (st = resolve_host_ties(ctx, hC, K, nt, ls.xslab, ls.xcnt, sums1)) != QVQ_OK) return st;
    }
    ls.upd = sums_out && !fused;
    if (ls.upd && !early_upd) {
        HIPCHK(hipEventRecord(ctx->ev[slot][2], ctx->stream));
        if ((st = run_update_slabs(ctx, p, ctx->ts.d_A, K, ls.nslabs)) != QVQ_OK) return st;
        HIPCHK(hipEventRecord(ctx->ev[slot][3], ctx->stream));
    }
    return QVQ_OK;
}

// The sums of the assignment run_level just made (ls), reduced into d_sums: the slabs together
// with the level's kd-tree ties (kd_reduce_kernel: their moves go to copy 1, which the finalize
// adds), or the slabs alone; no slabs: the sums are in d_sums already.  A tie count that run_level
// left to be published goes out with the slab reduce.  rs: what the finalize adds.
qvq_status reduce_level(qvq_ctx *ctx, uint32_t K, int slot, const LevelSums &ls, ReducedSums &rs) {
    const unsigned *tcnt = ctx->d_counters + 2 * slot + 1;   // the level's ties
    rs.copies = ls.copies;
    rs.gate = ls.copies > 1 ? tcnt : nullptr;
    if (ls.kd_pend) {
        mark_sums1(ctx);
        HIPCHK(launch_kd_reduce(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, ctx->ts.D, ctx->ts.d_ties, tcnt, ctx->lv.d_C64_split, K,
                                ctx->d_lut64, ls.kd, ctx->ts.d_A, ctx->d_plut, ctx->lv.d_part, ctx->lv.d_part_cnt,
                                ls.nslabs, ls.nsub, ctx->lv.d_sums, ctx->lv.d_sums + sums_cap_stride(ctx)));
    } else if (ls.nslabs) {
        HIPCHK(launch_reduce(ctx->stream, ctx->lv.d_part, ctx->lv.d_part_cnt, ls.nslabs, ls.nsub, K, ctx->ts.D, ctx->lv.d_sums, ls.pub));
    }
    if (ls.pub.flag && (ls.kd_pend || !ls.nslabs))   // the slab reduce did not run: a launch of its own
        HIPCHK(launch_copy_out(ctx->stream, ls.pub.cnt, ls.pub.dst, 4, nullptr, nullptr, 0, nullptr, nullptr, 0,
                               ls.pub.flag, ls.pub.seq, ctx->d_counters + COPY_DONE_COUNTER));
    return QVQ_OK;
}

// |c_kahan - c_exact| per split component for SCALED values (the tie band's delta)
constexpr double KAHAN_DELTA = 0x1p-49;

// The ties of a Kahan level answered from the level's own tree (over the exact-sum split) and
// the reference's sums of the few cells that can matter: the reference's search
// replayed over every split the certificate allows (RefKDTree::certified_search), first with
// what is known without sums; for the rows it leaves open, the reference's Kahan centroids of
// their candidates' parent cells (every code vector within a slack of the nearest that covers
// the reference's bits; the selected cells only), the replay again; for rows still open, the
// cells of the points a collecting replay blames, and once more.  done = false, nothing
// changed, when a row stays open: the caller then computes the whole split and its tree.
uint32_t cert_threads();
// The threads a check may use: cert_threads() (one while the main thread builds a kd-tree made
// the builds faster but the checks later: C4 6.88 vs 6.52 ms, profiles/r05z).
uint32_t cert_helpers(const qvq_ctx *) { return cert_threads(); }


// QVQ_CERT_TRACE=1: the certificate's phases, us since the check saw its level's export
struct CertTrace {
    bool on = false;
    std::chrono::steady_clock::time_point t0;
    std::string s;
    void mark(const char *what) {
        if (!on) return;
        char b[64];
        std::snprintf(b, sizeof(b), " %s %.0f", what,
                      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        s += b;
    }
};
thread_local CertTrace cert_trace;

// The split rows of the cells cell_of (their reference bits, [2][S][D]: slot | S + slot) into a
// certificate's known split; the tree's replay caches updated for those points.
void cert_apply_cells(const RefKDTree &tree, CertState &cs, uint32_t Kc, uint32_t D, const std::vector<uint32_t> &cell_of,
                      const double *split) {
    const uint32_t S = (uint32_t)cell_of.size();
    std::vector<uint32_t> changed;
    for (uint32_t t = 0; t < S; t++)
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t r = cell_of[t] + h * Kc;
            std::memcpy(&cs.kp[(size_t)r * D], &split[((size_t)h * S + t) * D], D * 8);
            std::memset(&cs.known[(size_t)r * D], 1, D);
            changed.push_back(r);
        }
    tree.cert_update(changed.data(), changed.size());   // kp / known changed on these rows
    cs.rounds++;
}

// fn(t) for t = 0 .. n - 1: t = 0 on the calling thread, the others on the pool's threads
// (for replays of tens of us and more: a helper's wake-up costs about that).  A job is one
// epoch: a helper reads the epoch, want and fn together under the lock, so it runs each epoch
// at most once and never a stale fn; a helper spawned now starts from the current epoch (it
// never sees a finished job as new).  The caller's fn(0) and the wait for busy == 0 keep every
// helper's fn(t) inside this call.
void pool_run(qvq_ctx *ctx, uint32_t n, const std::function<void(uint32_t)> &fn) {
    qvq_ctx::Pool &P = ctx->pool;
    if (n <= 1) {
        fn(0);
        return;
    }
    while (P.th.size() + 1 < n) {
        const uint32_t t = (uint32_t)P.th.size() + 1;
        uint64_t start;
        {
            std::lock_guard<std::mutex> g(P.m);
            start = P.epoch.load();
        }
        P.th.emplace_back([&P, t, start, dev = ctx->dev] {
            (void)hipSetDevice(dev);
            uint64_t seen = start;
            for (;;) {
                uint32_t want;
                std::function<void(uint32_t)> job;
                {
                    std::unique_lock<std::mutex> lk(P.m);
                    P.cv.wait(lk, [&] { return P.stop.load() || P.epoch.load() != seen; });
                    if (P.stop.load()) return;
                    seen = P.epoch.load();
                    want = P.want.load();
                    if (t < want) job = P.fn;
                }
                if (t < want) {
                    job(t);
                    P.busy.fetch_sub(1, std::memory_order_acq_rel);
                }
            }
        });
        if (ctx->place_ok) pthread_setaffinity_np(P.th.back().native_handle(), sizeof(cpu_set_t), &ctx->place);
    }
    {
        std::lock_guard<std::mutex> g(P.m);
        P.fn = fn;
        P.want.store(n);
        P.busy.store(n - 1);
        P.epoch.fetch_add(1);
    }
    P.cv.notify_all();
    fn(0);
    while (P.busy.load(std::memory_order_acquire)) std::this_thread::yield();
}

// The certificate's known split: coordinates whose reference bits are the exact sums' without
// computing them -- a cell's exact mean is 0 or 1 only when all its values are (SCALED values lie
// in [0, 1], at least 1/(255 n) from 1 otherwise; Kahan sums of 0s and 1s are exact), split by 1.2
// or 0.8, and every component of a cell of at most two rows (its Kahan sum, of one value or two,
// is the exact sum rounded once: the same centroid bits; pcnt, the finalize's parent counts).
// The tree's replay caches are reset for it; with prepare also built (the aggregates and every
// node's replayed split: the last level's check does this before its tie rows arrive).
// par (optional): the rows and the aggregates over the certificate's helper threads (the last
// level's check sets up a K = 4096, D = 48 certificate after its tree: ~0.5 ms on one thread)
void cert_init(const RefKDTree &tree, CertState &cs, const double *cb, const std::vector<uint32_t> &pcnt, uint32_t K,
               uint32_t D, bool prepare, qvq_ctx *par = nullptr) {
    const uint32_t Kc = K / 2;
    cs.kp.resize((size_t)K * D);
    cs.known.resize((size_t)K * D);
    const bool counts = pcnt.size() == Kc;
    auto rows = [&](uint32_t j0, uint32_t j1) {
        std::memcpy(&cs.kp[(size_t)j0 * D], cb + (size_t)j0 * D, (size_t)(j1 - j0) * D * 8);
        for (uint32_t j = j0; j < j1; j++) {
            const double u = j < Kc ? 1 + 0.2 : 1 - 0.2;
            const double *v = &cs.kp[(size_t)j * D];
            uint8_t *k = &cs.known[(size_t)j * D];
            const bool few = counts && pcnt[j % Kc] <= 2;
            for (uint32_t d = 0; d < D; d++) k[d] = few || v[d] == 0 || std::fabs(v[d] - u) <= 1e-14;
        }
    };
    const uint32_t nt = par && (uint64_t)K * D >= 65536 ? std::min<uint32_t>(cert_helpers(par), 8) : 1;
    if (nt > 1)
        pool_run(par, nt, [&](uint32_t t) { rows((uint32_t)((uint64_t)K * t / nt), (uint32_t)((uint64_t)K * (t + 1) / nt)); });
    else
        rows(0, K);
    tree.cert_clear();   // kp / known: this level's (the vectors are reused)
    if (prepare) tree.cert_prepare(KAHAN_DELTA, cs.kp.data(), cs.known.data());
    cs.prepared = true;
}

// The certificate over cs.nu distinct rows cs.qs (nu x D values): cs.ans[u] the reference's
// index, or -1 for a row it leaves open.  tree: the level's tree over the exact-sum split cb (K
// code vectors); A_prev: the previous level's assignment (nullptr at K = 2: the parent cell is the
// mean of every row), whose selected cells are summed on stream (sync waits for them).
// defer (several ranks): a cell's rows are split over the ranks, so no cell is
// summed here: the rows the known coordinates leave open stay in cs.pend with every cell they
// need in cs.sel (their candidates' and the blamed points'), and cert_finish completes them once
// the ranks have summed those cells together (qvq_lbg).
template <class Sync>
qvq_status certify_rows(qvq_ctx *ctx, const RefKDTree &tree, const double *cb, const std::vector<uint32_t> &pcnt,
                        uint32_t K, const uint32_t *A_prev, hipStream_t stream, Sync sync, CertState &cs, bool defer,
                        uint32_t &open_rows) {
    const uint32_t D = ctx->ts.D, Kc = K / 2, nu = cs.nu;
    const std::vector<double> &qs = cs.qs;
    std::vector<int64_t> &ans = cs.ans;
    if (!cs.prepared) cert_init(tree, cs, cb, pcnt, K, D, false);
    std::vector<double> &kp = cs.kp;
    std::vector<uint8_t> &known = cs.known;
    ans.assign(nu, -1);
    cs.pend.clear();
    cs.sel.assign(Kc, 0);
    // rows over host threads when the replays are long (48-D: the search visits most leaves)
    const bool long_search = (uint64_t)K * D >= 65536;   // 48-D: a search visits most leaves
    const uint32_t nthr = long_search ? std::min<uint32_t>(nu, cert_threads()) : 1;   // (the most)
    auto each = [&](const std::vector<uint32_t> &rows, auto &&fn) {   // fn(u, thread slot)
        // (per phase: one thread while the main thread builds a tree, cert_helpers)
        const uint32_t nthr = long_search ? std::min<uint32_t>(nu, cert_helpers(ctx)) : 1;
        if (nthr <= 1 || rows.size() < 2) {
            for (uint32_t u : rows) fn(u, 0u);
            return;
        }
        std::atomic<size_t> next{0};
        pool_run(ctx, std::min<uint32_t>(nthr, (uint32_t)rows.size()), [&](uint32_t t) {
            for (size_t i = next++; i < rows.size(); i = next++) fn(rows[i], t);
        });
    };
    std::vector<uint32_t> open, left;
    auto replay = [&](const std::vector<uint32_t> &rows) {
        each(rows, [&](uint32_t u, uint32_t) {
            ans[u] = tree.certified_search(&qs[(size_t)u * D], KAHAN_DELTA, kp.data(), known.data());
        });
        left.clear();
        for (uint32_t u : rows)
            if (ans[u] < 0) left.push_back(u);
        open.swap(left);
    };
    // each row's candidates (every code vector within a slack of the nearest that covers the
    // reference's bits); short searches replay every row at once and list candidates for the
    // rows left open only, long ones (48-D) replay at once only rows whose candidates are known
    std::vector<std::vector<uint32_t>> cand(nu);
    std::vector<uint32_t> all(nu);
    for (uint32_t u = 0; u < nu; u++) all[u] = u;
    auto near = [&](const std::vector<uint32_t> &rows) {
        each(rows, [&](uint32_t u, uint32_t) {
            double dmin;
            tree.near_set(&qs[(size_t)u * D], 1e-9, 1e-9, cand[u], dmin);
        });
        cert_trace.mark("near");
    };
    auto all_known = [&](uint32_t j) {
        for (uint32_t d = 0; d < D; d++)
            if (!known[(size_t)j * D + d]) return false;
        return true;
    };
    std::vector<uint32_t> ready, &pend = cs.pend;
    // long searches (48-D) list candidates first and skip the replays their unknown candidates
    // doom; short ones replay first and list candidates for the rows left open only (C3's last
    // level: 2 rows, near sets 36 us of a 53 us check after the export, profiles/r05p)
    const bool near_first = long_search;
    if (near_first) {
        near(all);
        for (uint32_t u = 0; u < nu; u++) {
            bool k = true;
            for (uint32_t j : cand[u]) k = k && all_known(j);
            (k ? ready : pend).push_back(u);
        }
    } else {
        ready = all;
    }
    if (!ready.empty()) {
        replay(ready);
        pend.insert(pend.end(), open.begin(), open.end());
        cert_trace.mark("replay");
        if (!near_first) near(pend);
    }
    std::vector<uint8_t> &sel = cs.sel;
    cs.cells = cs.rounds = 0;
    auto want = [&](uint32_t j) {
        if (all_known(j)) return;
        cs.cells += !sel[j % Kc];
        sel[j % Kc] = 1;
    };
    // the reference's centroids of the selected cells (of the previous level's assignment),
    // compacted to slots; the split rows (slot | S + slot) land in mapped host memory
    std::vector<uint32_t> cell_of;
    auto launch_cells = [&](const std::vector<uint8_t> &pick) -> qvq_status {
        qvq_status s2;
        if ((s2 = ensure_kahan(ctx, Kc)) != QVQ_OK) return s2;
        cell_of.clear();
        for (uint32_t c = 0; c < Kc; c++) {
            ctx->kh.cells.h_kc_sel[c] = pick[c] ? (uint32_t)cell_of.size() + 1 : 0u;
            if (pick[c]) cell_of.push_back(c);
        }
        if (A_prev) {
            // the longest chain (the finalize's parent counts): short ones run step by step
            uint64_t max_rows = pcnt.size() == Kc ? 1 : 0;
            for (uint32_t c : cell_of) max_rows = max_rows ? std::max<uint64_t>(max_rows, pcnt[c]) : 0;
            HIPCHK(hipMemcpyAsync(ctx->kh.cells.d_kc_sel, ctx->kh.cells.h_kc_sel, (size_t)Kc * 4, hipMemcpyHostToDevice, stream));
            HIPCHK(launch_kahan_centroids(stream, ctx->kh.kw, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.N, A_prev,
                                          (uint32_t)cell_of.size(), ctx->kh.cells.d_kc_cent, ctx->kh.cells.h_kc_out.dev(), ctx->kh.cells.d_kc_sel, Kc,
                                          max_rows));
        } else {   // K = 2: the one parent cell is the mean of every row
            HIPCHK(launch_kahan_centroids(stream, ctx->kh.kw, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.N, nullptr, 1,
                                          ctx->kh.cells.d_kc_cent, ctx->kh.cells.h_kc_out.dev(), nullptr, 0, ctx->ts.N));
        }
        cert_trace.mark("launched");
        return QVQ_OK;
    };
    auto finish_cells = [&]() -> qvq_status {
        qvq_status s2;
        if ((s2 = sync()) != QVQ_OK) return s2;
        cert_trace.mark("sums");
        cert_apply_cells(tree, cs, Kc, D, cell_of, ctx->kh.cells.h_kc_out);
        return QVQ_OK;
    };
    open.clear();
    if (!pend.empty() && (K >= 4 ? A_prev != nullptr : K == 2)) {
        // the candidates' cells on the GPU while a collecting replay finds the points whose bits
        // settle the decisions the intervals leave open (with the candidates unknown, it blames
        // them too); their cells, if new, in a second round
        qvq_status st;
        for (uint32_t u : pend)
            for (uint32_t j : cand[u]) want(j);
        std::vector<uint8_t> first = sel;
        if (cs.cells && !defer && (st = launch_cells(first)) != QVQ_OK) return st;
        std::vector<std::vector<uint32_t>> blame(std::max<uint32_t>(nthr, 1));
        each(pend, [&](uint32_t u, uint32_t t) {
            tree.certify_blame(&qs[(size_t)u * D], KAHAN_DELTA, kp.data(), known.data(), blame[t]);
        });
        const uint32_t c0 = cs.cells;
        for (const auto &b : blame)
            for (uint32_t j : b) want(j);
        cert_trace.mark("blame");
        if (defer) {   // the cells come from every rank's rows (cert_finish)
            open_rows = (uint32_t)pend.size();
            return QVQ_OK;
        }
        if (c0 && (st = finish_cells()) != QVQ_OK) return st;
        if (cs.cells > c0) {
            std::vector<uint8_t> more(Kc, 0);
            for (uint32_t c = 0; c < Kc; c++) more[c] = sel[c] && !first[c];
            if ((st = launch_cells(more)) != QVQ_OK || (st = finish_cells()) != QVQ_OK) return st;
        }
        replay(pend);
        cert_trace.mark("replay");
    } else {
        open = pend;
    }
    pend = open;
    open_rows = (uint32_t)open.size();
    return QVQ_OK;
}

// The deferred rows (certify_rows with defer) once the cells cell_of have their reference bits:
// split rows at split ([2][S][D]: slot | S + slot); returns the rows still open.
uint32_t cert_finish(const RefKDTree &tree, CertState &cs, uint32_t K, uint32_t D, const std::vector<uint32_t> &cell_of,
                     const double *split) {
    cert_apply_cells(tree, cs, K / 2, D, cell_of, split);
    tree.cert_clear();   // (every thread's cache: the replays run here, the defer's ran elsewhere)
    std::vector<uint32_t> open;
    for (uint32_t u : cs.pend) {
        cs.ans[u] = tree.certified_search(&cs.qs[(size_t)u * D], KAHAN_DELTA, cs.kp.data(), cs.known.data());
        if (cs.ans[u] < 0) open.push_back(u);
    }
    cs.pend.swap(open);
    return (uint32_t)cs.pend.size();
}

// A settled row whose reference index is not its speculative one (the quantize must be redone).
bool cert_mismatch(const CertState &cs, uint32_t K) {
    for (size_t i = 0; i < cs.rows.size(); i++) {
        const int64_t a = cs.ans[cs.of[i]];
        if (a >= 0 && (uint32_t)a != cs.spec[i]) {
            if (env_is("QVQ_KAHAN_DEBUG", "1"))
                std::fprintf(stderr, "qvq kahan: K %u row %u: speculative %u, the reference %lld\n", K, cs.rows[i],
                             cs.spec[i], (long long)a);
            return true;
        }
    }
    return false;
}

// Host threads for the certificate's replays (at most 8, half the machine's).
uint32_t cert_threads() {
    static const uint32_t n = [] {
        // (C4 at 1 / 2 / 4 / 8 helpers is within the boxes' run-to-run spread, 6.8-7.6 ms:
        // profiles/r05s, r05u)
        return std::max<uint32_t>(1, std::min<uint32_t>(8, std::thread::hardware_concurrency() / 2));
    }();
    return n;
}

// Distinct rows of n row records (code bytes at code + i * stride, D of them): their values qs,
// and of[i] = the distinct row of record i.
uint32_t distinct_rows(const qvq_ctx *ctx, const uint8_t *code, size_t stride, uint32_t n, std::vector<double> &qs,
                       std::vector<uint32_t> &of) {
    std::unordered_map<std::string, uint32_t> uniq;
    of.resize(n);
    qs.clear();
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *c = code + (size_t)i * stride;
        const auto it = uniq.emplace(std::string(reinterpret_cast<const char *>(c), ctx->ts.D), (uint32_t)uniq.size());
        of[i] = it.first->second;
        if (it.second)
            for (uint32_t d = 0; d < ctx->ts.D; d++) qs.push_back(ctx->ts.terms.v64[c[d]]);
    }
    return (uint32_t)uniq.size();
}

qvq_status certify_kahan_ties(qvq_ctx *ctx, uint32_t K, unsigned nt, uint64_t *target, bool &done) {
    done = false;
    if (!ctx->tree || ctx->cb_local.size() != (size_t)K * ctx->ts.D || K < 2) return QVQ_OK;
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t need = (uint64_t)nt * (4 + Dp);
    HIPCHK(ctx->d_scatter.ensure(need / 4));
    uint32_t *d_vals = ctx->d_scatter;
    uint8_t *d_gath = reinterpret_cast<uint8_t *>(ctx->d_scatter + nt);
    std::vector<uint8_t> code((uint64_t)nt * Dp);
    HIPCHK(launch_gather_codes(ctx->stream, ctx->ts.d_codes, Dp, ctx->ts.d_ties, nt, d_gath));
    HIPCHK(hipMemcpyAsync(code.data(), d_gath, code.size(), hipMemcpyDeviceToHost, ctx->stream));
    qvq_status st;
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    CertState cs;
    cs.nu = distinct_rows(ctx, code.data(), Dp, nt, cs.qs, cs.of);
    uint32_t open = 0;
    if ((st = certify_rows(ctx, *ctx->tree, ctx->cb_local.data(), ctx->cnt_local, K, K == 2 ? nullptr : ctx->ts.d_A_alt, ctx->stream,
                           [ctx] { return wait_stream(ctx); }, cs, false, open)) != QVQ_OK)
        return st;
    if (open) {
        if (env_is("QVQ_KAHAN_DEBUG", "1"))
            std::fprintf(stderr, "qvq kahan: K %u ties %u (%u distinct) cells %u: %u rows not certified\n", K, nt, cs.nu,
                         cs.cells, open);
        return QVQ_OK;
    }
    std::vector<uint32_t> &vals = ctx->cert_vals;   // outlives the copy (no wait)
    vals.resize(nt);
    for (uint32_t i = 0; i < nt; i++) vals[i] = (uint32_t)cs.ans[cs.of[i]];
    HIPCHK(hipMemcpyAsync(d_vals, vals.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_fix_rows(ctx->stream, ctx->ts.d_codes, Dp, D, ctx->ts.d_A, ctx->ts.d_ties, d_vals, nt, K, nullptr, nullptr,
                           ctx->d_plut, target));
    if (env_is("QVQ_KAHAN_DEBUG", "1"))
        std::fprintf(stderr, "qvq kahan: K %u ties %u (%u distinct) certified, cells summed %u in %u rounds\n", K, nt,
                     cs.nu, cs.cells, cs.rounds);
    done = true;
    return QVQ_OK;
}

// The speculative check of one level (on the worker): the level's tie rows and their
// speculative indices (exported with its codebook) against the reference's, by the certificate
// over the level's tree.  status 0: all equal; 1: a row differs or stays open (qvq_lbg then
// redoes the quantize with the synchronous Kahan levels); 2 (several ranks): the rows settled
// so far agree and the rest wait for cells summed over every rank's rows (v.cs, cert_finish).
// QVQ_KAHAN_FAIL_LEVEL=L (tests): level L's check fails (on rank QVQ_KAHAN_FAIL_RANK, default
// every rank), exercising the redo.
void verify_level(qvq_ctx *ctx, qvq_ctx::Verify &v) {
    v.status = 1;
    ctx->htrace.mark("check K" + std::to_string(v.K) + " start");
    struct End {
        qvq_ctx *c;
        const qvq_ctx::Verify &v;
        ~End() { c->htrace.mark("check K" + std::to_string(v.K) + " end, status " + std::to_string(v.status)); }
    } end_mark{ctx, v};
    (void)hipSetDevice(ctx->dev);
    // the check usually starts while the GPU still runs its level (the last level's check is
    // then all that is left of the call): the known split and the tree's aggregates before the
    // export arrives, and for short searches (D = 12: a few hundred nodes) every node's split
    // replay too (C3: the last level's 2 tie rows took ~95 us after the export, r05i)
    // (C3 1.241 -> 1.197 ms, C4 7.51 -> 7.18, profiles/r05p)
    if (!v.cs.prepared && v.tree && !v.tree->cancelled() && v.K >= 2 &&
        v.cb.size() == (size_t)v.K * ctx->ts.D) {
        const bool full = (uint64_t)v.K * ctx->ts.D < 65536;
        cert_init(*v.tree, v.cs, v.cb.data(), v.cnt, v.K, ctx->ts.D, full, ctx);
        ctx->htrace.mark("check K" + std::to_string(v.K) + " known split set");
        if (!full)
            v.tree->cert_warm(KAHAN_DELTA, v.cs.kp.data(), v.cs.known.data(), cert_helpers(ctx),
                              [ctx](unsigned n, const std::function<void(unsigned)> &fn) { pool_run(ctx, n, fn); });
        ctx->htrace.mark("check K" + std::to_string(v.K) + " aggregates set");
    }
    volatile uint64_t *flag = ctx->h_ready;
    while (*flag < v.seq) {   // the export is released with the codebook's ready number
        if (v.cancel.load(std::memory_order_relaxed)) return;
        cpu_relax();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    ctx->htrace.mark("check K" + std::to_string(v.K) + " export seen");
    static const int fail_level = std::getenv("QVQ_KAHAN_FAIL_LEVEL") ? std::atoi(std::getenv("QVQ_KAHAN_FAIL_LEVEL")) : 0;
    static const int fail_rank = std::getenv("QVQ_KAHAN_FAIL_RANK") ? std::atoi(std::getenv("QVQ_KAHAN_FAIL_RANK")) : -1;
    if (fail_level && (int)v.level == fail_level && (fail_rank < 0 || fail_rank == ctx->rank)) return;
    static const bool trace = env_is("QVQ_CERT_TRACE", "1");
    cert_trace.on = trace;
    cert_trace.t0 = std::chrono::steady_clock::now();
    cert_trace.s.clear();
    const uint32_t *tx = reinterpret_cast<const uint32_t *>(ctx->h_tx[v.par].get());
    const uint32_t nt = tx[0];
    if (nt == 0) {
        v.status = 0;
        return;
    }
    if (nt > ctx->tx_cap) {
        ctx->tm.tie_overflow++;
        return;
    }
    if (!v.tree || v.tree->cancelled() || v.K < 2) return;
    const uint32_t Dp = ctx->ts.Dp, words = 2 + Dp / 4;
    std::vector<uint32_t> rec(tx + 2, tx + 2 + (size_t)nt * words);   // out of the mapped buffer at once
    CertState &cs = v.cs;
    cs.rows.resize(nt);
    cs.spec.resize(nt);
    for (uint32_t i = 0; i < nt; i++) {
        cs.rows[i] = rec[(size_t)i * words];
        cs.spec[i] = rec[(size_t)i * words + 1];
        if (cs.rows[i] >= ctx->ts.N || cs.spec[i] >= v.K) return;
    }
    cs.nu = distinct_rows(ctx, reinterpret_cast<const uint8_t *>(rec.data() + 2), (size_t)words * 4, nt, cs.qs, cs.of);
    uint32_t open = 0;
    // the selected cells' sums on the check's stream: a bounded poll that also ends when the
    // call cancels the check (a failed wait in qvq_lbg), so joining a cancelled check is prompt
    auto sync = [ctx, &v]() -> qvq_status {
        const auto until = std::chrono::steady_clock::now() + std::chrono::duration<double>(ctx->timeout_s);
        for (;;) {
            const hipError_t q = hipStreamQuery(ctx->vstream);
            if (q == hipSuccess) return QVQ_OK;
            if (q != hipErrorNotReady) return QVQ_EDEVICE;
            if (v.cancel.load(std::memory_order_relaxed) || std::chrono::steady_clock::now() > until)
                return QVQ_EDEVICE;
            std::this_thread::yield();
        }
    };
    const bool defer = ctx->nranks > 1;
    // (A_prev is complete: the GPU wrote the flag seen above after the levels that made it)
    if (certify_rows(ctx, *v.tree, v.cb.data(), v.cnt, v.K, v.A_prev, ctx->vstream, sync, cs, defer, open) != QVQ_OK ||
        (open && !defer))
        return;
    // QVQ_KAHAN_OPEN_LEVEL=L (tests; -1: every level): a row of level L left open with no cell
    // wanted, on rank QVQ_KAHAN_FAIL_RANK (default every rank) -- the state that no later sum can
    // settle, which must end in the redo
    static const int open_level = std::getenv("QVQ_KAHAN_OPEN_LEVEL") ? std::atoi(std::getenv("QVQ_KAHAN_OPEN_LEVEL")) : 0;
    if (open_level && (open_level < 0 || (int)v.level == open_level) && (fail_rank < 0 || fail_rank == ctx->rank) &&
        cs.nu > 0) {
        if (cs.pend.empty()) cs.pend.push_back(0);
        open = (uint32_t)cs.pend.size();
        cs.sel.assign(v.K / 2, 0);
        cs.cells = 0;
    }
    // open rows that want no cell (their candidates all known, yet a decision left open): no
    // cell summed over the ranks can settle them, so the level fails here (several ranks: a
    // deferred entry without cells would be skipped by resolve_deferred, keeping unconfirmed
    // speculative indices)
    if (open && cs.cells == 0) return;
    if (cert_mismatch(cs, v.K)) return;
    cert_trace.mark("done");
    if (env_is("QVQ_KAHAN_DEBUG", "1") || trace)
        std::fprintf(stderr, "qvq kahan: K %u ties %u (%u distinct) %s, cells %s %u in %u rounds%s%s\n", v.K, nt, cs.nu,
                     open ? "deferred" : "verified", open ? "wanted" : "summed", cs.cells, cs.rounds,
                     trace ? " | us:" : "", cert_trace.s.c_str());
    v.status = open ? 2 : 0;
}

// The check's verdict (status 0 / 1 / 2, -1: none posted); its tree and rows are released,
// except a deferred check's (status 2, several ranks), which moves to ctx->kh.deferred.

// free_on_worker: the check's tree and state are destroyed on the worker, not here (the last
// level's at the end of a call: C4's K = 4096 tree and certificate free ~30 us of buffers, with
// the munmaps' TLB shootdowns, while the caller waits)
int join_verify(qvq_ctx *ctx, qvq_ctx::Verify &v, bool free_on_worker = false) {
    if (!v.posted) return -1;
    while (!v.done.load(std::memory_order_acquire)) std::this_thread::yield();
    v.posted = false;
    const int status = v.status;
    if (status == 2) {
        qvq_ctx::Kahan::Deferred d;
        d.level = v.level;
        d.K = v.K;
        d.A_prev = v.A_prev;
        d.tree = std::move(v.tree);
        d.cb = std::move(v.cb);
        d.cs = std::move(v.cs);
        ctx->kh.deferred.push_back(std::move(d));
    }
    if (free_on_worker && v.tree) {
        RefKDTree *t = v.tree.release();
        CertState *c = new CertState(std::move(v.cs));
        post_job(ctx, [t, c] {
            delete t;
            delete c;
        }, nullptr);
    }
    v.tree.reset();
    v.cs = CertState();
    return status;
}

// join_verify within the context's wait bounds: a failed stream or communicator, or a timeout,
// fails the call as any other wait does (wait_failed; a drained stream is no failure here: the
// check's host replays may outlast the GPU's work).  ok = not failed (status 0, 2 or none).
qvq_status join_verify_bounded(qvq_ctx *ctx, qvq_ctx::Verify &v, bool &ok, bool free_on_worker = false) {
    ok = true;
    if (!v.posted) return QVQ_OK;
    std::string err;
    const qvq_status st = wait_until(
        [&] { return v.done.load(std::memory_order_acquire); },
        [&](std::string &m) {
            const StreamState ss = probe_stream(ctx, m);
            return ss == StreamState::Drained ? StreamState::Running : ss;
        },
        [&](std::string &m) { return probe_comm(ctx, m); }, ctx->timeout_s, err);
    if (st != QVQ_OK) {
        for (auto &u : ctx->ver) u.cancel.store(true);
        return wait_failed(ctx, fail(ctx, st, err));
    }
    ok = join_verify(ctx, v, free_on_worker) != 1;
    return QVQ_OK;
}

// The speculative check's buffers: four assignment buffers (per training set), once per context
// the mapped tie exports, the check's stream and events, and the Kahan work for the largest level.
qvq_status ensure_speculation(qvq_ctx *ctx, uint32_t Kmax) {
    qvq_status st = ensure_apool(ctx, ctx->ts, 4);
    if (st != QVQ_OK) return st;
    ctx->tx_cap = 65536;
    for (auto &h : ctx->h_tx) HIPCHK(h.ensure(8 + (size_t)ctx->tx_cap * (8 + 64)));
    if (!ctx->vstream) {   // high priority: the check's few short kernels go ahead of the next search's queued blocks
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
            HIPCHK(hipStreamCreateWithPriority(ctx->vstream.put(), hipStreamNonBlocking, hi));
        else
            HIPCHK(hipStreamCreateWithFlags(ctx->vstream.put(), hipStreamNonBlocking));
    }
    for (auto &v : ctx->ver)
        if (!v.ev) HIPCHK(hipEventCreateWithFlags(v.ev.put(), hipEventDisableTiming));
    return Kmax >= 4 ? ensure_kahan(ctx, Kmax / 2) : QVQ_OK;
}

// The nt tie rows of a level (in d_ties) answered against the reference's split S_ref (device;
// copied to h_kc_split): the level's own tree (over the exact-sum split, built during the
// search) is the reference's tree too when no differing coordinate can move a box, cut or
// partition (kdtree.cpp); otherwise a tree over the host copy, or the host's answers where there
// is no device image.  The rows' terms move within the sums at target.
qvq_status answer_kahan_ties(qvq_ctx *ctx, const LevelPlan &p, uint32_t K, int slot, unsigned nt, const double *S_ref,
                             uint64_t *target) {
    const uint32_t D = ctx->ts.D;
    ctx->h_kc_split.resize((size_t)K * D);
    HIPCHK(hipMemcpyAsync(ctx->h_kc_split.data(), S_ref, (size_t)K * D * 8, hipMemcpyDeviceToHost, ctx->stream));
    const qvq_status st = wait_stream(ctx);
    if (st != QVQ_OK || nt == 0) return st;
    KdView kd;
    if (ctx->tree && ctx->tree_kd.depth > 0 && ctx->cb_local.size() == (size_t)K * D &&
        ctx->tree->unchanged_under(ctx->h_kc_split.data())) {
        kd = ctx->tree_kd;
        if (env_is("QVQ_KAHAN_DEBUG", "1")) std::fprintf(stderr, "qvq kahan: K %u the level's tree reused\n", K);
    } else {
        build_tree(ctx, p, ctx->h_kc_split.data(), K, slot & 1, kd);
    }
    if (kd.depth > 0) {
        HIPCHK(launch_kd_resolve(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.d_ties, ctx->d_counters + 2 * slot + 1, S_ref,
                                 K, ctx->d_lut64, kd, ctx->ts.d_A, nullptr, nullptr, ctx->d_plut, target));
        return QVQ_OK;
    }
    return resolve_host_ties(ctx, ctx->h_kc_split.data(), K, nt, nullptr, nullptr, target);
}

// The ties of a level run with defer_ties (nt > 0 of them in d_ties): the reference's split
// codebook -- the previous level's centroids as Kahan sums in row order (k_kahan.hip; for the
// NORMAL colour space the exact sums are those bits already), split -- its kd-tree, and the
// ties answered against both (every distance recomputed from the reference's code vectors).
// The moves go to sums copy 1 (a fusable level: rs then has the finalize add it) or straight
// into copy 0.
qvq_status resolve_kahan_ties(qvq_ctx *ctx, const LevelPlan &p, uint32_t K, int slot, unsigned nt, ReducedSums &rs) {
    const uint32_t D = ctx->ts.D, Kc = K / 2;
    const double *S_ref = ctx->lv.d_C64_split;
    qvq_status st;
    uint64_t *target = ctx->lv.d_sums;
    rs = ReducedSums();
    if (p.fusable) {
        mark_sums1(ctx);
        target += sums_cap_stride(ctx);
        rs.copies = 2;
        rs.gate = ctx->d_counters + 2 * slot + 1;
    }
    if (ctx->ts.cs == QVQ_CS_SCALED) {
        bool done;
        if ((st = certify_kahan_ties(ctx, K, nt, target, done)) != QVQ_OK || done) return st;
        if ((st = ensure_kahan(ctx, Kc)) != QVQ_OK) return st;
        HIPCHK(launch_kahan_centroids(ctx->stream, ctx->kh.kw, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.N,
                                      K == 2 ? nullptr : ctx->ts.d_A_alt, Kc, ctx->kh.cells.d_kc_cent, ctx->kh.cells.d_kc_split));
        S_ref = ctx->kh.cells.d_kc_split;
        if (env_is("QVQ_KAHAN_DEBUG", "1")) {   // blocks not composable, block misses, segment replays
            unsigned ms[4];
            HIPCHK(hipMemcpyAsync(ms, ctx->kh.kw.stats, sizeof(ms), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemsetAsync(ctx->kh.kw.stats, 0, sizeof(ms), ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            std::fprintf(stderr, "qvq kahan: K %u level ties %u blocks not composable %u block misses %u replays %u\n",
                         K, nt, ms[0], ms[1], ms[2]);
        }
    }
    return answer_kahan_ties(ctx, p, K, slot, nt, S_ref, target);
}

// resolve_kahan_ties on several ranks (a level with ties on any rank, every rank calls it): the
// reference's whole split from the chains over every rank's rows (kahan_chained), its kd-tree,
// this rank's ties (nt) answered against both, and the ties' moves of every rank summed (sums
// copy 1, added by the finalize that follows: rs, without a gate).
qvq_status resolve_kahan_ties_multi(qvq_ctx *ctx, const LevelPlan &p, uint32_t K, int slot, unsigned nt,
                                    ReducedSums &rs) {
    const uint32_t Kc = K / 2;
    qvq_status st;
    mark_sums1(ctx);
    uint64_t *target = ctx->lv.d_sums + sums_cap_stride(ctx);
    rs = ReducedSums();
    rs.copies = 2;
    if ((st = kahan_chained(ctx, K == 2 ? nullptr : ctx->ts.d_A_alt, Kc, nullptr, Kc, true)) != QVQ_OK) return st;
    if ((st = answer_kahan_ties(ctx, p, K, slot, nt, ctx->kh.cells.d_kc_split, target)) != QVQ_OK) return st;
    return all_reduce_sums(ctx, K, target);
}

// Several ranks, at the end of a speculative qvq_lbg: the checks whose rows wait
// for cells summed over every rank's rows (ctx->kh.deferred).  A vote of every rank's failure and,
// per level, of the cells its open rows need; then for each level with cells wanted (ascending,
// every rank the same), their reference bits from the chains over every rank's rows
// (kahan_chained on the level's parent assignment, alev[L - 1]) and this rank's open rows
// replayed with them (cert_finish); a second vote of the failures.  failed: in, this rank's
// failure so far; out, any rank's (the quantize is then redone on every rank).
qvq_status resolve_deferred(qvq_ctx *ctx, uint32_t bits, const std::vector<uint32_t *> &alev, bool &failed) {
    const uint32_t D = ctx->ts.D;
    // [0] failures | per level L: its parent cells (2^(L-1)), four 16-bit counts per word
    std::vector<uint64_t> off(bits + 2, 1);
    for (uint32_t L = 1; L <= bits; L++) off[L + 1] = off[L] + ((1ull << (L - 1)) + 3) / 4;
    std::vector<uint64_t> v(off[bits + 1], 0);
    v[0] = failed ? 1 : 0;
    for (const auto &d : ctx->kh.deferred)
        for (uint32_t c = 0; c < d.K / 2; c++)
            if (d.cs.sel[c]) v[off[d.level] + c / 4] |= 1ull << (16 * (c % 4));
    qvq_status st;
    if ((st = vote(ctx, v.data(), v.size())) != QVQ_OK) return st;
    if (v[0]) {
        failed = true;
        return QVQ_OK;
    }
    bool local_fail = false;
    std::vector<uint32_t> cell_of;
    std::vector<double> split;
    for (uint32_t L = 1; L <= bits; L++) {
        const uint32_t Kc = 1u << (L - 1);
        cell_of.clear();
        for (uint32_t c = 0; c < Kc; c++)
            if ((v[off[L] + c / 4] >> (16 * (c % 4))) & 0xFFFF) cell_of.push_back(c);
        if (cell_of.empty()) {   // no rank wants a cell here: rows still open stay open (a redo)
            for (const auto &d : ctx->kh.deferred)
                if (d.level == L && !d.cs.pend.empty()) local_fail = true;
            continue;
        }
        ctx->tm.kahan_relays++;
        const uint32_t S = (uint32_t)cell_of.size();
        if ((st = ensure_kahan(ctx, Kc)) != QVQ_OK) return st;
        if (L >= 2) {
            for (uint32_t c = 0; c < Kc; c++) ctx->kh.cells.h_kc_sel[c] = 0;
            for (uint32_t t = 0; t < S; t++) ctx->kh.cells.h_kc_sel[cell_of[t]] = t + 1;
            HIPCHK(hipMemcpyAsync(ctx->kh.cells.d_kc_sel, ctx->kh.cells.h_kc_sel, (size_t)Kc * 4, hipMemcpyHostToDevice, ctx->stream));
            st = kahan_chained(ctx, alev[L - 1], Kc, ctx->kh.cells.d_kc_sel, S, true);
        } else {
            st = kahan_chained(ctx, nullptr, 1, nullptr, 1, true);
        }
        if (st != QVQ_OK) return st;
        split.resize(2ull * S * D);
        HIPCHK(hipMemcpyAsync(split.data(), ctx->kh.cells.d_kc_split, split.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((st = wait_stream(ctx)) != QVQ_OK) return st;
        for (auto &d : ctx->kh.deferred) {
            if (d.level != L) continue;
            const uint32_t open = cert_finish(*d.tree, d.cs, d.K, D, cell_of, split.data());
            const bool bad = open || cert_mismatch(d.cs, d.K);
            if (env_is("QVQ_KAHAN_DEBUG", "1"))
                std::fprintf(stderr, "qvq kahan: rank %d K %u deferred rows finished over %u cells: %s\n", ctx->rank,
                             d.K, S, open ? "rows left open" : bad ? "a row differs" : "verified");
            local_fail = local_fail || bad;
        }
    }
    uint64_t f = local_fail ? 1 : 0;
    if ((st = vote(ctx, &f, 1)) != QVQ_OK) return st;
    failed = f != 0;
    return QVQ_OK;
}

// The byte histogram of the resident rows (kept on the device: qvq_lbg derives sum ||x||^2 and
// the row count from it, after summing it over the ranks).
qvq_status compute_xsq(qvq_ctx *ctx) {
    HIPCHK(launch_byte_hist(ctx->stream, ctx->ts.d_codes, ctx->ts.N, ctx->ts.D, ctx->ts.Dp, ctx->d_hist));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return QVQ_OK;
}

qvq_status check_image_args(qvq_ctx *ctx, uint32_t n_images, uint32_t xSize, uint32_t ySize, uint32_t bw,
                            uint32_t bh, uint64_t &N, uint32_t &D) {
    if (!ctx) return QVQ_EINVAL;
    if (n_images == 0 || xSize == 0 || ySize == 0 || bw == 0 || bh == 0)
        return fail(ctx, QVQ_EINVAL, "image and block sizes must be positive");
    N = (uint64_t)((xSize + bw - 1) / bw) * ((ySize + bh - 1) / bh) * n_images;
    D = 3 * bw * bh;
    return QVQ_OK;
}

qvq_status tile_into(qvq_ctx *ctx, const uint8_t *d_rgb, uint32_t n_images, uint32_t xSize, uint32_t ySize,
                     uint32_t bw, uint32_t bh) {
    ctx->col_blocks = (ySize + bh - 1) / bh;   // the pruned wide search stacks its chunks across columns
    HIPCHK(launch_tile(ctx->stream, d_rgb, ctx->ts.d_codes, n_images, xSize, ySize, bw, bh, ctx->ts.D, ctx->ts.Dp,
                       ctx->ts.terms.pad_code));
    return QVQ_OK;
}

// What a CIE1931 raster must pass after check_image_args, in this order, before the resident set is
// touched: its values are no byte images, so it becomes an exact-mode set.
qvq_status check_cie_raster(qvq_ctx *ctx, uint64_t N, uint32_t bw, uint32_t bh) {
    if (bw > 64 || bh > 64 || 3 * bw * bh > 64)
        return fail(ctx, QVQ_EINVAL, "block dimension above 64 (3*w*h) is not supported");
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "CIE1931 values are not byte images (exact mode runs on one rank)");
    if (N >= (1ull << 31)) return fail(ctx, QVQ_EINVAL, "exact mode: more than 2^31-1 rows");
    return QVQ_OK;
}

}  // namespace

extern "C" {

// Exact mode's training set (which sets take it: "way 2" below), ahead of the entry points that
// install one.
// The exact-mode set of n rows of dim components: adopt (an upload of the engine's own) taken over
// as d_X64 as it is, or a fresh d_X64 that fill writes with work on the context's stream (a copy of
// the caller's rows, or the launch that produces them).  raster_cs: the colour space of the raster
// the rows come from, -1 for fp64 rows (qvq_get_training_info).  Returns with the stream drained.
static qvq_status install_exact(qvq_ctx *ctx, uint64_t n, uint32_t dim, int raster_cs, DevBuf<double> *adopt,
                                const std::function<hipError_t(double *)> &fill) {
    ctx->rf = qvq_ctx::RefineState();
    drop_training(ctx);   // before the new set's allocations: peak memory is one set
    qvq_ctx::Training ts;   // moved into the context when it is complete
    ts.N = n;
    ts.D = dim;
    ts.Dp = (dim + 3) & ~3u;
    ts.exact = true;
    ts.exact_cs = raster_cs;
    if (adopt) ts.ex.d_X64 = std::move(*adopt);
    else HIPCHK(ts.ex.d_X64.alloc(n * dim));
    qvq_status st = ensure_apool(ctx, ts, 1);
    if (st != QVQ_OK) return st;
    HIPCHK(ts.d_ties.alloc(n));
    HIPCHK(ts.ex.d_keys.alloc(n));
    HIPCHK(ts.ex.d_iota.alloc(n));
    HIPCHK(ts.ex.d_order.alloc(n));
    ts.ex.temp_bytes = exact_sort_temp_bytes(n);
    HIPCHK(ts.ex.d_temp.alloc(std::max<size_t>(ts.ex.temp_bytes, 16)));
    if (!adopt) HIPCHK(fill(ts.ex.d_X64));
    HIPCHK(launch_exact_iota(ctx->stream, ts.ex.d_iota, n));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->ts = std::move(ts);
    return QVQ_OK;
}
// ... from src's rows: on the host, or on the device where the context's stream may read them
static qvq_status install_exact_copy(qvq_ctx *ctx, const double *src, hipMemcpyKind kind, DevBuf<double> *adopt, uint64_t n,
                                     uint32_t dim) {
    return install_exact(ctx, n, dim, -1, adopt, [&](double *dst) {
        return hipMemcpyAsync(dst, src, n * dim * 8, kind, ctx->stream);
    });
}
// ... from the rasters d_rgb (device memory the context's stream may read) under CIE1931, tiled
// and converted in one launch (k_tile64.hip): nothing is classified -- the values are never byte
// images -- and nothing is copied: the launch writes d_X64.  Under
// qvq_set_timing(-3) events around the launch give its device ms (qvq_get_ingest_ms()[1]).
static qvq_status install_cie_raster(qvq_ctx *ctx, const uint8_t *d_rgb, uint32_t n_images, uint32_t xSize,
                                     uint32_t ySize, uint32_t bw, uint32_t bh, uint64_t N, uint32_t D) {
    const bool timed = ctx->timing_level == -3;
    ctx->ingest_ms[0] = ctx->ingest_ms[1] = 0;
    const qvq_status st = install_exact(ctx, N, D, QVQ_CS_CIE1931, nullptr, [&](double *dst) {
        hipError_t e = timed ? hipEventRecord(ctx->ev_ing[1], ctx->stream) : hipSuccess;
        if (e == hipSuccess) e = launch_tile64(ctx->stream, d_rgb, dst, n_images, xSize, ySize, bw, bh);
        if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev_ing[2], ctx->stream);
        return e;
    });
    float ms = 0;
    if (st == QVQ_OK && timed && hipEventElapsedTime(&ms, ctx->ev_ing[1], ctx->ev_ing[2]) == hipSuccess)
        ctx->ingest_ms[1] = ms;
    return st;
}

QVQ_API const char *qvq_version(void) { return "qvq 0.2 (gfx950, f16 MFMA search)"; }

QVQ_API const char *qvq_last_error(const qvq_ctx *ctx) { return ctx ? ctx->err.c_str() : g_static_err.c_str(); }

QVQ_API qvq_status qvq_create(int hip_device, qvq_ctx **out) {
    if (!out) return QVQ_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(nullptr, QVQ_EDEVICE, "no HIP device");
    if (hip_device < 0 || hip_device >= n) return fail(nullptr, QVQ_EINVAL, "bad device index");
    std::unique_ptr<qvq_ctx> owner(new qvq_ctx());   // an early return destroys what was made
    qvq_ctx *ctx = owner.get();
    ctx->dev = hip_device;
    if (const char *t = std::getenv("QVQ_TIMING")) ctx->timing_level = std::atoi(t);   // A/B: the default per-level events
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    // (errors go to the thread's static string: the caller gets no context to ask)
#define CREATECHK(expr, what)                                                                          \
    do {                                                                                               \
        const hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(nullptr, QVQ_EDEVICE, std::string(what) + ": " + hipGetErrorString(e_)); \
    } while (0)
    CREATECHK(hipSetDevice(hip_device), "hipSetDevice");
    hipDeviceProp_t prop;
    CREATECHK(hipGetDeviceProperties(&prop, hip_device), "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, QVQ_EDEVICE, std::string("libqvq is built for gfx950, device is ") + prop.gcnArchName);
    ctx->num_cu = prop.multiProcessorCount;
    ctx->G = (uint32_t)ctx->num_cu;   // one search/update workgroup (and slab) per CU
    CREATECHK(hipStreamCreateWithFlags(ctx->stream.put(), hipStreamNonBlocking), "stream");
    CREATECHK(ctx->d_lut32.alloc(256), "hipMalloc");
    CREATECHK(ctx->d_w.alloc(256), "hipMalloc");
    CREATECHK(ctx->d_lut64.alloc(256), "hipMalloc");
    CREATECHK(ctx->d_plut.alloc(256), "hipMalloc");
    CREATECHK(ctx->h_ready.alloc(1024 / 8), "hipHostMalloc");
    *ctx->h_ready = 0;
    CREATECHK(ctx->d_counters.alloc(N_COUNTERS_ALLOC), "hipMalloc");
    CREATECHK(hipMemset(ctx->d_counters, 0, ctx->d_counters.bytes()), "hipMemset");
    CREATECHK(ctx->d_hist.alloc(512), "hipMalloc");
    CREATECHK(ctx->d_decode_stat.alloc(2), "hipMalloc");
    CREATECHK(ctx->h_decode_stat.alloc(2), "hipHostMalloc");
    CREATECHK(ctx->d_dist_part.alloc(8192), "hipMalloc");
    CREATECHK(ctx->d_mean.alloc(MEAN_COPIES * (2 * 64 + 1)), "hipMalloc");
    CREATECHK(hipMemset(ctx->d_mean, 0, ctx->d_mean.bytes()), "hipMemset");
    for (auto &level : ctx->ev)
        for (Event &ev : level) CREATECHK(hipEventCreate(ev.put()), "hipEventCreate");
    CREATECHK(hipEventCreate(ctx->ev_end.put()), "hipEventCreate");
    CREATECHK(hipEventCreateWithFlags(ctx->ev_sync.put(), hipEventDisableTiming), "hipEventCreate");
    {
        std::vector<double> tab(512);
        for (int cs : {QVQ_CS_NORMAL, QVQ_CS_SCALED}) {
            Terms t;
            make_terms(cs, t);
            std::memcpy(&tab[256 * cs], t.v64, sizeof(t.v64));
        }
        CREATECHK(ctx->d_ing_tab.alloc(512), "hipMalloc");
        CREATECHK(hipMemcpy(ctx->d_ing_tab, tab.data(), 512 * 8, hipMemcpyHostToDevice), "hipMemcpy");
        CREATECHK(ctx->d_ing_verdict.alloc(1), "hipMalloc");
        CREATECHK(ctx->h_ing_verdict.alloc(1), "hipHostMalloc");
        for (Event &ev : ctx->ev_ing) CREATECHK(hipEventCreate(ev.put()), "hipEventCreate");
    }
#undef CREATECHK
    if (const char *t = std::getenv("QVQ_TIMEOUT_S")) ctx->timeout_s = std::max(0.001, std::atof(t));
    *out = owner.release();
    return QVQ_OK;
}

// The ordered part of the teardown: no thread or queued work may outlive the buffers, which the
// context's members then release (streams last: they are declared first).
QVQ_API void qvq_destroy(qvq_ctx *ctx) {
    if (!ctx) return;
    join_tree_job(ctx, true);
    for (auto &v : ctx->ver) v.cancel.store(true);
    while (ctx->worker.pending.load(std::memory_order_acquire)) std::this_thread::yield();
    {
        std::lock_guard<std::mutex> g(ctx->pool.m);
        ctx->pool.stop.store(true);
    }
    ctx->pool.cv.notify_all();
    for (auto &t : ctx->pool.th) t.join();
    {
        qvq_ctx::Worker *w = &ctx->worker;
        if (w->th.joinable()) {
            {
                std::lock_guard<std::mutex> g(w->m);
                w->stop = true;
            }
            w->cv.notify_one();
            w->th.join();
        }
    }
    (void)hipSetDevice(ctx->dev);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->kstream) (void)hipStreamSynchronize(ctx->kstream);
    if (ctx->comm) ncclCommDestroy(ctx->comm);
    delete ctx;
}

QVQ_API uint64_t qvq_num_vectors(const qvq_ctx *ctx) { return ctx ? ctx->ts.N : 0; }
QVQ_API uint32_t qvq_dim(const qvq_ctx *ctx) { return ctx ? ctx->ts.D : 0; }
QVQ_API const uint32_t *qvq_assign_device(const qvq_ctx *ctx) { return ctx ? ctx->ts.d_A : nullptr; }

QVQ_API qvq_status qvq_set_images_device(qvq_ctx *ctx, const void *d_rgb, uint32_t n_images, uint32_t xSize,
                                         uint32_t ySize, uint32_t bw, uint32_t bh, int colorspace) {
    uint64_t N;
    uint32_t D;
    qvq_status st = check_image_args(ctx, n_images, xSize, ySize, bw, bh, N, D);
    if (st != QVQ_OK) return st;
    GUARD(ctx);
    if (!d_rgb) return fail(ctx, QVQ_EINVAL, "null raster");
    if (colorspace == QVQ_CS_CIE1931 && (st = check_cie_raster(ctx, N, bw, bh)) != QVQ_OK) return st;
    HIPCHK(hipSetDevice(ctx->dev));
    if (colorspace == QVQ_CS_CIE1931)
        return install_cie_raster(ctx, (const uint8_t *)d_rgb, n_images, xSize, ySize, bw, bh, N, D);
    if ((st = alloc_training(ctx, N, D, colorspace)) != QVQ_OK) return st;
    if ((st = tile_into(ctx, (const uint8_t *)d_rgb, n_images, xSize, ySize, bw, bh)) != QVQ_OK) return st;
    return compute_xsq(ctx);
}

QVQ_API qvq_status qvq_set_images(qvq_ctx *ctx, const uint8_t *rgb, uint32_t n_images, uint32_t xSize, uint32_t ySize,
                                  uint32_t bw, uint32_t bh, int colorspace) {
    uint64_t N;
    uint32_t D;
    qvq_status st = check_image_args(ctx, n_images, xSize, ySize, bw, bh, N, D);
    if (st != QVQ_OK) return st;
    GUARD(ctx);
    if (!rgb) return fail(ctx, QVQ_EINVAL, "null raster");
    if (colorspace == QVQ_CS_CIE1931 && (st = check_cie_raster(ctx, N, bw, bh)) != QVQ_OK) return st;
    HIPCHK(hipSetDevice(ctx->dev));
    const uint64_t bytes = (uint64_t)xSize * ySize * 3 * n_images;
    HIPCHK(ctx->d_raster.ensure(bytes));   // kept across calls (repeated compresses)
    const hipError_t e = host_copy(ctx, ctx->d_raster, rgb, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, QVQ_EDEVICE, std::string("raster upload: ") + hipGetErrorString(e));
    if (colorspace == QVQ_CS_CIE1931)
        return install_cie_raster(ctx, ctx->d_raster, n_images, xSize, ySize, bw, bh, N, D);
    if ((st = alloc_training(ctx, N, D, colorspace)) != QVQ_OK) return st;
    if ((st = tile_into(ctx, ctx->d_raster, n_images, xSize, ySize, bw, bh)) != QVQ_OK) return st;
    return compute_xsq(ctx);
}

QVQ_API qvq_status qvq_set_synthetic(qvq_ctx *ctx, uint32_t S, uint64_t seed0, uint32_t n_images, uint32_t bw,
                                     uint32_t bh, int colorspace) {
    uint64_t N;
    uint32_t D;
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (S < 2) return fail(ctx, QVQ_EINVAL, "synthetic images need S >= 2");
    qvq_status st = check_image_args(ctx, n_images, S, S, bw, bh, N, D);
    if (st != QVQ_OK) return st;
    const bool cie = colorspace == QVQ_CS_CIE1931;
    if (cie && (st = check_cie_raster(ctx, N, bw, bh)) != QVQ_OK) return st;
    HIPCHK(hipSetDevice(ctx->dev));
    const uint64_t npix = (uint64_t)S * S * n_images;
    DevBuf<uint8_t> d_rgb;   // (freed after the synchronize below)
    HIPCHK(d_rgb.alloc(npix * 3));
    st = QVQ_OK;
    const hipError_t e = launch_gen(ctx->stream, d_rgb, S, seed0, npix);
    if (e != hipSuccess) st = fail(ctx, QVQ_EDEVICE, std::string("gen_kernel: ") + hipGetErrorString(e));
    if (st == QVQ_OK && cie) st = install_cie_raster(ctx, d_rgb, n_images, S, S, bw, bh, N, D);
    if (st == QVQ_OK && !cie) st = alloc_training(ctx, N, D, colorspace);
    if (st == QVQ_OK && !cie) st = tile_into(ctx, d_rgb, n_images, S, S, bw, bh);
    if (st == QVQ_OK && !cie) st = compute_xsq(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    return st;
}

// ---------------------------------------------------------------------------------------
// Training set, way 2: fp64 rows.  Which mode a set takes is decided by the rule of
// byte_image.hpp over every value: SCALED if the whole set is SCALED-valid, otherwise NORMAL if
// the whole set is NORMAL-valid, otherwise exact mode (k_exact.hip: any finite fp64 data, the
// reference's arithmetic bit for bit -- fp64 search in nanoflann's order with kd-tree ties, Kahan
// sums over each cell's rows in ascending order times fl(1/n), src/Quantizer.cpp:46-87; one rank,
// host-driven levels).  The rule runs on the device (k_ingest.hip: classify, then pack; DESIGN.md
// 3.12) over rows that are already there (qvq_set_vectors_device) or that the host entry points
// upload once; the host form of the rule (host_classify) is the fallback when that upload's buffer
// cannot be allocated, and qvq_host_classify.
// ---------------------------------------------------------------------------------------

// The rule over a host array: the colour space (-1: not a byte image), *finite = no Inf / NaN
// (complete whenever the answer is -1), and the codes [n][Dp] (codes may be null) of a byte image.
static int host_classify(const double *X, uint64_t n, uint32_t dim, uint8_t *codes, bool *finite) {
    Terms ts, tn;
    make_terms(QVQ_CS_SCALED, ts);
    make_terms(QVQ_CS_NORMAL, tn);
    bool sc = true, nm = true, fin = true;
    const uint64_t total = n * dim;
    for (uint64_t i = 0; i < total && (sc || nm || fin); i++) {
        const double v = X[i];
        sc = sc && byte_image_code(v, true, ts.v64) >= 0;
        nm = nm && byte_image_code(v, false, tn.v64) >= 0;
        fin = fin && f64_finite(v);
    }
    if (finite) *finite = fin;
    const int cs = sc ? QVQ_CS_SCALED : nm ? QVQ_CS_NORMAL : -1;
    if (cs >= 0 && codes) {
        const Terms &t = sc ? ts : tn;
        const uint32_t Dp = (dim + 3) & ~3u;
        for (uint64_t i = 0; i < n; i++) {
            for (uint32_t d = 0; d < dim; d++) codes[i * Dp + d] = (uint8_t)byte_image_code(X[i * dim + d], sc, t.v64);
            for (uint32_t d = dim; d < Dp; d++) codes[i * Dp + d] = t.pad_code;
        }
    }
    return cs;
}

// The checks every fp64 entry point makes before it touches a value.
static qvq_status check_vector_args(qvq_ctx *ctx, const void *X, uint64_t n, uint32_t dim, bool exact) {
    if (!X || n == 0 || dim == 0) return fail(ctx, QVQ_EINVAL, "empty training set");
    if (dim > 64) return fail(ctx, QVQ_EINVAL, "block dimension above 64 (3*w*h) is not supported");
    if (exact && n >= (1ull << 31)) return fail(ctx, QVQ_EINVAL, "exact mode: more than 2^31-1 rows");
    if (n >= (1ull << 32)) return fail(ctx, QVQ_EINVAL, "more than 2^32-1 rows per rank");
    return QVQ_OK;
}

// What a set that is no byte image (or is forced to exact mode) must pass, in this order, before the
// resident set is touched.
static qvq_status check_exact_set(qvq_ctx *ctx, uint64_t n, bool forced, bool finite) {
    // one rank only -- with a communicator the ranks would disagree on the mode: fail fast here
    // instead of at qvq_lbg, where peers would wait in the first all-reduce
    if (!forced && (ctx->comm || ctx->host_ar))
        return fail(ctx, QVQ_EUNSUPPORTED, "values are not byte images (exact mode runs on one rank)");
    if (n >= (1ull << 31)) return fail(ctx, QVQ_EINVAL, "exact mode: more than 2^31-1 rows");
    if (!finite) return fail(ctx, QVQ_EINVAL, "exact mode: training values must be finite");
    return QVQ_OK;
}

// The training set from fp64 rows dX [n][dim] that the context's stream may read: classify, then
// pack under the space found or install the rows as the exact-mode set.  adopt: dX is *adopt, the
// engine's own upload, which exact mode keeps.  Returns with the stream drained.
static qvq_status ingest_rows(qvq_ctx *ctx, const double *dX, uint64_t n, uint32_t dim, bool force_exact,
                              DevBuf<double> *adopt) {
    const bool timed = ctx->timing_level == -3;   // events around the two passes (qvq_get_ingest_ms)
    ctx->ingest_ms[0] = ctx->ingest_ms[1] = 0;
    if (timed) HIPCHK(hipEventRecord(ctx->ev_ing[0], ctx->stream));
    HIPCHK(launch_ingest_classify(ctx->stream, dX, n, dim, ctx->d_ing_tab, ctx->d_ing_verdict));
    if (timed) HIPCHK(hipEventRecord(ctx->ev_ing[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_ing_verdict, ctx->d_ing_verdict, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const unsigned v = *ctx->h_ing_verdict;
    float ms = 0;
    if (timed && hipEventElapsedTime(&ms, ctx->ev_ing[0], ctx->ev_ing[1]) == hipSuccess) ctx->ingest_ms[0] = ms;
    const int cs = force_exact ? -1 : (v & ING_SCALED_OK) ? QVQ_CS_SCALED : (v & ING_NORMAL_OK) ? QVQ_CS_NORMAL : -1;
    qvq_status st;
    if (cs < 0) {
        if ((st = check_exact_set(ctx, n, force_exact, (v & ING_FINITE) != 0)) != QVQ_OK) return st;
        return install_exact_copy(ctx, dX, hipMemcpyDeviceToDevice, adopt, n, dim);
    }
    ctx->col_blocks = 0;   // rows without image geometry
    // (the same shape again keeps every buffer; the pack below refills d_codes either way)
    if ((st = alloc_training(ctx, n, dim, cs)) != QVQ_OK) return st;
    if (timed) HIPCHK(hipEventRecord(ctx->ev_ing[1], ctx->stream));
    HIPCHK(launch_ingest_pack(ctx->stream, dX, n, dim, (uint32_t)cs, ctx->d_ing_tab, ctx->ts.d_codes));
    if (timed) HIPCHK(hipEventRecord(ctx->ev_ing[2], ctx->stream));
    if ((st = compute_xsq(ctx)) != QVQ_OK) return st;
    if (timed && hipEventElapsedTime(&ms, ctx->ev_ing[1], ctx->ev_ing[2]) == hipSuccess) ctx->ingest_ms[1] = ms;
    return QVQ_OK;
}

// The same from a host array without the transient upload (its allocation failed): the host form
// of the rule, then the codes' or the rows' upload.
static qvq_status ingest_host_rule(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim, bool force_exact) {
    ctx->ingest_ms[0] = ctx->ingest_ms[1] = 0;
    const uint32_t Dp = (dim + 3) & ~3u;
    std::vector<uint8_t> codes;
    if (!force_exact) codes.resize(n * Dp);
    bool finite = true;
    int cs = -1;
    if (force_exact)
        for (uint64_t i = 0; i < n * dim && finite; i++) finite = f64_finite(X[i]);
    else
        cs = host_classify(X, n, dim, codes.data(), &finite);
    qvq_status st;
    if (cs < 0) {
        if ((st = check_exact_set(ctx, n, force_exact, finite)) != QVQ_OK) return st;
        return install_exact_copy(ctx, X, hipMemcpyHostToDevice, nullptr, n, dim);
    }
    ctx->col_blocks = 0;
    if ((st = alloc_training(ctx, n, dim, cs)) != QVQ_OK) return st;
    HIPCHK(hipMemcpy(ctx->ts.d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice));
    return compute_xsq(ctx);
}

static qvq_status set_vectors_host(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim, bool force_exact) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    qvq_status st = check_vector_args(ctx, X, n, dim, force_exact);
    if (st != QVQ_OK) return st;
    HIPCHK(hipSetDevice(ctx->dev));
    // one upload into a transient buffer: the pass reads it, exact mode keeps it as d_X64
    DevBuf<double> rows;
    if (rows.alloc(n * dim) != hipSuccess) {
        (void)hipGetLastError();
        return ingest_host_rule(ctx, X, n, dim, force_exact);
    }
    HIPCHK(hipMemcpyAsync(rows, X, n * dim * 8, hipMemcpyHostToDevice, ctx->stream));
    return ingest_rows(ctx, rows, n, dim, force_exact, &rows);
}

QVQ_API qvq_status qvq_set_vectors(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim) {
    return set_vectors_host(ctx, X, n, dim, false);
}

QVQ_API qvq_status qvq_set_vectors_exact(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim) {
    return set_vectors_host(ctx, X, n, dim, true);
}

QVQ_API qvq_status qvq_set_vectors_device(qvq_ctx *ctx, const void *d_X, uint64_t n, uint32_t dim, uint32_t flags,
                                          void *stream) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (flags & ~(uint32_t)QVQ_VECTORS_EXACT) return fail(ctx, QVQ_EINVAL, "unknown flags");
    const bool force_exact = (flags & QVQ_VECTORS_EXACT) != 0;
    qvq_status st = check_vector_args(ctx, d_X, n, dim, force_exact);
    if (st != QVQ_OK) return st;
    if ((uintptr_t)d_X % 8) return fail(ctx, QVQ_EINVAL, "rows not 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->dev));
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, d_X) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->dev) {
        (void)hipGetLastError();
        return fail(ctx, QVQ_EINVAL, "rows are not device memory on the context's GPU");
    }
    // ordered after the work that produces the rows: the engine's stream waits for what the
    // caller's stream holds now (the mirror image of qvq_decode_device)
    HIPCHK(hipEventRecord(ctx->ev_sync, (hipStream_t)stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_sync, 0));
    return ingest_rows(ctx, (const double *)d_X, n, dim, force_exact, nullptr);
}

QVQ_API qvq_status qvq_get_training_info(const qvq_ctx *ctx, qvq_training_info *out) {
    if (!ctx || !out) return QVQ_EINVAL;
    out->mode = ctx->ts.exact ? 2u : ctx->ts.d_codes ? 1u : 0u;
    out->colorspace = out->mode == 1 ? ctx->ts.cs : out->mode == 2 ? ctx->ts.exact_cs : -1;
    out->n = ctx->ts.N;
    out->dim = ctx->ts.D;
    return QVQ_OK;
}

// The resident rows row0 .. row0 + nrows - 1 as fp64 [nrows][dim]: exact mode's rows themselves, or the
// byte path's codes through the colour space's table (rows_f64_kernel into the decode scratch).  In
// pieces of at most GET_PIECE bytes through pinned staging: a piece reaches the caller's memory only
// after the bounded wait for its copy has succeeded.
QVQ_API qvq_status qvq_get_vectors(qvq_ctx *ctx, uint64_t row0, uint64_t nrows, double *out) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (!out || nrows == 0) return fail(ctx, QVQ_EINVAL, "empty read-back");
    if (row0 >= ctx->ts.N || nrows > ctx->ts.N - row0) return fail(ctx, QVQ_EINVAL, "rows outside the training set");
    HIPCHK(hipSetDevice(ctx->dev));
    constexpr uint64_t GET_PIECE = 64ull << 20;
    const uint64_t row_bytes = (uint64_t)ctx->ts.D * 8;
    const uint64_t piece_rows = std::min<uint64_t>(nrows, std::max<uint64_t>(1, GET_PIECE / row_bytes));
    HIPCHK(ctx->h_stage.ensure(piece_rows * row_bytes));
    qvq_status st;
    if (!ctx->ts.exact) HIPCHK(ctx->d_decode.ensure(piece_rows * row_bytes));
    for (uint64_t r = 0; r < nrows; r += piece_rows) {
        const uint64_t nr = std::min(piece_rows, nrows - r);
        const double *src = ctx->ts.ex.d_X64 + (row0 + r) * ctx->ts.D;
        if (!ctx->ts.exact) {
            double *d = reinterpret_cast<double *>(ctx->d_decode.get());
            HIPCHK(launch_rows_f64(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, ctx->ts.D, row0 + r, nr, ctx->d_lut64, d));
            src = d;
        }
        HIPCHK(hipMemcpyAsync(ctx->h_stage, src, nr * row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if ((st = wait_stream(ctx)) != QVQ_OK) return st;
        std::memcpy(out + r * ctx->ts.D, ctx->h_stage, nr * row_bytes);
    }
    return QVQ_OK;
}

QVQ_API qvq_status qvq_get_ingest_ms(const qvq_ctx *ctx, double ms[2]) {
    if (!ctx || !ms) return QVQ_EINVAL;
    ms[0] = ctx->ingest_ms[0];
    ms[1] = ctx->ingest_ms[1];
    return QVQ_OK;
}

// Exact mode's host-driven levels (k_exact.hip) ---------------------------------------------
namespace {

qvq_status exact_single_rank(qvq_ctx *ctx) {
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "exact mode runs on one rank (Kahan sums do not split across ranks)");
    return QVQ_OK;
}

qvq_status exact_koff(qvq_ctx *ctx, uint32_t K) {
    HIPCHK(ctx->ts.ex.d_koff.ensure((size_t)K + 1));
    return QVQ_OK;
}

// Assignment of every row against the K code vectors at d_C64_split (host copy hC): the
// fp64 argmin, exact ties answered by the host kd-tree over hC.  Returns the tie count.
qvq_status exact_assign(qvq_ctx *ctx, const double *hC, uint32_t K, unsigned &nties) {
    const uint32_t D = ctx->ts.D;
    qvq_status st;
    unsigned *cnt = ctx->d_counters + 1;
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned), ctx->stream));
    HIPCHK(launch_exact_assign(ctx->stream, ctx->ts.ex.d_X64, ctx->ts.N, D, ctx->lv.d_C64_split, K, 1e-12, ctx->ts.d_A, ctx->ts.d_ties,
                               cnt));
    HIPCHK(hipMemcpyAsync(&nties, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    if (nties == 0) return QVQ_OK;
    const uint64_t need = (uint64_t)nties * (8 + 8ull * D);
    HIPCHK(ctx->d_scatter.ensure(need / 4));
    uint32_t *d_vals = ctx->d_scatter;
    double *d_rows = reinterpret_cast<double *>(ctx->d_scatter + 2 * (uint64_t)nties);
    std::vector<uint32_t> rows(nties), vals(nties);
    std::vector<double> q((size_t)nties * D);
    HIPCHK(launch_exact_gather(ctx->stream, ctx->ts.ex.d_X64, D, ctx->ts.d_ties, nties, d_rows));
    HIPCHK(hipMemcpyAsync(rows.data(), ctx->ts.d_ties, nties * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(q.data(), d_rows, q.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    RefKDTree tree(hC, K, (int)D);
    for (unsigned i = 0; i < nties; i++) vals[i] = tree.nearest(q.data() + (size_t)i * D);
    HIPCHK(hipMemcpyAsync(d_vals, vals.data(), nties * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_exact_fix(ctx->stream, ctx->ts.d_A, ctx->ts.d_ties, d_vals, nties));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;   // the host vectors must outlive the copies
    return QVQ_OK;
}

// Centroids of assignment d_A (nullptr: the mean) into d_C64_cent, counts into cnt (device, may be null).
qvq_status exact_centroids(qvq_ctx *ctx, bool mean, uint32_t K, uint64_t *cnt) {
    qvq_status st = exact_koff(ctx, K);
    if (st != QVQ_OK) return st;
    HIPCHK(launch_exact_centroids(ctx->stream, ctx->ts.ex.d_X64, ctx->ts.N, ctx->ts.D, mean ? nullptr : ctx->ts.d_A, K,
                                  ctx->ts.ex.d_keys, ctx->ts.ex.d_iota, ctx->ts.ex.d_order, ctx->ts.ex.d_koff, ctx->ts.ex.d_temp,
                                  ctx->ts.ex.temp_bytes, ctx->lv.d_C64_cent, cnt));
    return QVQ_OK;
}

qvq_status lbg_exact(qvq_ctx *ctx, uint32_t bits, double *codebook, uint32_t *assign, double *distortion) {
    qvq_status st = exact_single_rank(ctx);
    if (st != QVQ_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t Kmax = 1u << bits, D = ctx->ts.D;
    if ((st = ensure_levels(ctx, std::max<uint32_t>(Kmax, 2))) != QVQ_OK) return st;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    ctx->tm.levels = (int)bits;
    // codeVectors[0] = trainingSetSum() / N (src/Quantizer.cpp:129-130)
    std::vector<double> hC((size_t)Kmax * D), hS((size_t)Kmax * D);
    if ((st = exact_centroids(ctx, true, 1, nullptr)) != QVQ_OK) return st;
    HIPCHK(hipMemcpyAsync(hC.data(), ctx->lv.d_C64_cent, (size_t)D * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    if (bits == 0) HIPCHK(hipMemsetAsync(ctx->ts.d_A, 0, ctx->ts.N * 4, ctx->stream));
    for (uint32_t lvl = 1; lvl <= bits; lvl++) {
        const uint32_t K = 1u << lvl, H = K / 2;
        // concat(C, C), then the halves scaled by (1 + 0.2) and (1 - 0.2) (src/Quantizer.cpp:134-138)
        for (size_t i = 0; i < (size_t)H * D; i++) {
            hS[i] = hC[i] * (double)(1 + 0.2);
            hS[(size_t)H * D + i] = hC[i] * (double)(1 - 0.2);
        }
        HIPCHK(hipMemcpyAsync(ctx->lv.d_C64_split, hS.data(), (size_t)K * D * 8, hipMemcpyHostToDevice, ctx->stream));
        unsigned nt = 0;
        const auto ta = std::chrono::steady_clock::now();
        if ((st = exact_assign(ctx, hS.data(), K, nt)) != QVQ_OK) return st;   // synchronous
        const auto tb = std::chrono::steady_clock::now();
        ctx->tm.host_ties[lvl - 1] = nt;
        if ((st = exact_centroids(ctx, false, K, nullptr)) != QVQ_OK) return st;
        HIPCHK(hipMemcpyAsync(hC.data(), ctx->lv.d_C64_cent, (size_t)K * D * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((st = wait_stream(ctx)) != QVQ_OK) return st;
        // wall times: assign (search + ties) and update (sort + Kahan chains + codebook copy)
        ctx->tm.assign_ms[lvl - 1] = std::chrono::duration<float, std::milli>(tb - ta).count();
        ctx->tm.update_ms[lvl - 1] =
            std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tb).count();
    }
    // updateDistortion after the last fix (src/Quantizer.cpp:9-22)
    double dist = 0;
    HIPCHK(launch_exact_distortion(ctx->stream, ctx->ts.ex.d_X64, ctx->ts.N, D, ctx->lv.d_C64_cent, ctx->ts.d_A, ctx->d_dist_part,
                                   ctx->d_dist_part + 4096));
    // results reach the caller only after the bounded wait succeeds (staged in pinned memory)
    HIPCHK(ctx->h_stage.ensure(8 + (assign ? ctx->ts.N * 4 : 0)));
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    HIPCHK(hipMemcpyAsync(stage, ctx->d_dist_part + 4096, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (assign) HIPCHK(hipMemcpyAsync(stage + 8, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    std::memcpy(&dist, stage, 8);
    if (assign) std::memcpy(assign, stage + 8, ctx->ts.N * 4);
    if (codebook) std::memcpy(codebook, hC.data(), (size_t)Kmax * D * 8);
    if (distortion) *distortion = dist;
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return QVQ_OK;
}

}  // namespace

// Host placement, one rank: the engine's host threads -- the caller's for the duration of
// qvq_lbg, the worker and the certificate's helpers -- on the L3 domain (CCD, SMT siblings
// included) of the CPU the first quantize ran on, within the threads' allowed CPUs.  The level's
// tree build, its check and the helpers share the codebook, the tree and its caches; spread over
// the GPU box's 16 L3 domains, C4 ran ~0.4 ms slower (profiles/r07c: 6.84 vs 6.31-6.44 ms).
static bool l3_domain(int cpu, cpu_set_t &out) {
    char path[128];
    std::snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char buf[1024];
    const size_t n = std::fread(buf, 1, sizeof(buf) - 1, f);
    std::fclose(f);
    buf[n] = 0;
    CPU_ZERO(&out);
    const char *q = buf;
    while (*q) {   // "a-b,c,..."
        char *e;
        const long a = std::strtol(q, &e, 10);
        if (e == q) break;
        long b = a;
        q = e;
        if (*q == '-') {
            b = std::strtol(q + 1, &e, 10);
            if (e == q + 1) break;
            q = e;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (c >= 0) CPU_SET((int)c, &out);
        while (*q == ',' || *q == '\n' || *q == ' ') q++;
    }
    return CPU_COUNT(&out) > 0;
}

struct HostPlaceGuard {   // the caller's CPUs narrowed to ctx->place during one call
    bool set = false;
    cpu_set_t old;
    explicit HostPlaceGuard(qvq_ctx *ctx) {
        if (ctx->comm || ctx->host_ar) return;   // several ranks share the box's CPUs: left alone
        if (pthread_getaffinity_np(pthread_self(), sizeof(old), &old) != 0) return;
        if (!ctx->place_tried) {
            ctx->place_tried = true;
            cpu_set_t l3;
            const int cpu = sched_getcpu();
            if (cpu >= 0 && l3_domain(cpu, l3)) {
                CPU_AND(&ctx->place, &l3, &old);
                ctx->place_ok = CPU_COUNT(&ctx->place) > 0;
            }
            if (ctx->place_ok) {   // threads started before (the worker of an earlier call)
                if (ctx->worker.th.joinable())
                    pthread_setaffinity_np(ctx->worker.th.native_handle(), sizeof(cpu_set_t), &ctx->place);
                for (std::thread &t : ctx->pool.th)
                    pthread_setaffinity_np(t.native_handle(), sizeof(cpu_set_t), &ctx->place);
            }
        }
        if (!ctx->place_ok) return;
        cpu_set_t want;
        CPU_AND(&want, &old, &ctx->place);
        if (CPU_COUNT(&want) == 0) return;
        set = pthread_setaffinity_np(pthread_self(), sizeof(want), &want) == 0;
    }
    ~HostPlaceGuard() {
        if (set) pthread_setaffinity_np(pthread_self(), sizeof(old), &old);
    }
};

// A finished qvq_lbg's events and published counters into ctx->tm: per level the device times
// (upd: the level timed a separate sums pass, LevelSums::upd) and the flagged and tie rows (stats:
// the level counters as copy_out published them), and the mean kernel's time.
static void lbg_timings(qvq_ctx *ctx, uint32_t bits, const bool *upd, const unsigned *stats) {
    for (uint32_t lvl = 1; lvl <= bits; lvl++) {
        // assign: the search kernel; update: the non-fused update; other: the rest of the
        // level up to the next level's search (recheck, kd-tree, reduce, finalize, tables)
        float a = 0, u = 0, whole = 0;
        const bool timed = ctx->timing_level == -1 || ctx->timing_level == (int)lvl - 1;
        if (timed) {
            (void)hipEventSynchronize(ctx->ev[lvl - 1][1]);   // complete; the runtime may not know yet
            (void)hipEventElapsedTime(&a, ctx->ev[lvl - 1][0], ctx->ev[lvl - 1][1]);
        }
        if (upd[lvl - 1]) {
            (void)hipEventSynchronize(ctx->ev[lvl - 1][3]);
            (void)hipEventElapsedTime(&u, ctx->ev[lvl - 1][2], ctx->ev[lvl - 1][3]);
        }
        if (ctx->timing_level == -1) (void)hipEventSynchronize(ctx->ev_end);
        if (ctx->timing_level == -1)
            (void)hipEventElapsedTime(&whole, ctx->ev[lvl - 1][0], lvl < bits ? ctx->ev[lvl][0] : ctx->ev_end);
        ctx->tm.assign_ms[lvl - 1] = a;
        ctx->tm.other_ms[lvl - 1] = ctx->timing_level == -1 ? std::max(0.f, whole - a - u) : 0.f;
        ctx->tm.update_ms[lvl - 1] = u;
        ctx->tm.flagged[lvl - 1] = stats[2 * (lvl - 1)];
        ctx->tm.host_ties[lvl - 1] = stats[2 * (lvl - 1) + 1];
    }
    if (ctx->timing_level == -3) {
        float m = 0;
        (void)hipEventSynchronize(ctx->ev[31][1]);
        (void)hipEventElapsedTime(&m, ctx->ev[31][0], ctx->ev[31][1]);
        ctx->tm.mean_ms = m;
    }
}

QVQ_API qvq_status qvq_lbg(qvq_ctx *ctx, uint32_t bits, double eps, double *codebook, uint32_t *assign,
                           double *distortion) {
    (void)eps;   // cannot change the outputs: one Lloyd step per level
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (bits > 20) return fail(ctx, QVQ_EINVAL, "bits must be <= 20");
    ctx->rf.valid = false;
    HIPCHK(hipSetDevice(ctx->dev));
    if (ctx->ts.exact) return lbg_exact(ctx, bits, codebook, assign, distortion);
    const HostPlaceGuard place(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    static const bool htrace = env_is("QVQ_HOST_TRACE", "1");
    if (htrace) {
        ctx->htrace.start(t0);
    }
    const uint32_t Kmax = 1u << bits;
    qvq_status st = ensure_levels(ctx, std::max<uint32_t>(Kmax, 2));
    if (st != QVQ_OK) return st;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    ctx->tm.levels = (int)bits;
    // codeVectors[0] = trainingSetSum() / N, then the first split (src/Quantizer.cpp:129-138).
    // The mean kernel also clears the counters and writes [sum ||x||^2, rows] for the
    // closed-form distortion (summed over all ranks below).
    double *d_dist = ctx->d_dist_part;
    // sum ||x||^2 and the row count come from the byte histogram (qvq_set_*), all-reduced as
    // integers first: the distortion is then the same bits for every rank count
    const uint64_t *hist = ctx->d_hist;
    if (ctx->comm || ctx->host_ar) {
        HIPCHK(hipMemcpyAsync(ctx->d_hist + 256, ctx->d_hist, 256 * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if ((st = all_reduce(ctx, ctx->d_hist + 256, 256, false)) != QVQ_OK) return st;
        hist = ctx->d_hist + 256;
    }
    // Reference-bit (Kahan) levels, SCALED values (NORMAL values are integers: the exact sums are
    // the reference's bits).  Speculative (default): each level runs as with exact sums, its ties
    // answered by the exact-sum tree on the device, and the worker checks them against the
    // reference's rule (the certificate) while the GPU runs the next level; a
    // level whose check fails makes the quantize run again with synchronous Kahan levels (each
    // waits for its ties to be answered by the reference's rule).  Several ranks:
    // a check never sums a cell on its own (a cell's chain runs over every rank's rows); its open
    // rows wait for the end of the call, where the ranks vote, sum the cells wanted together
    // (kahan_chained) and vote again, so that every rank redoes the quantize or none does.
    // QVQ_SPECULATE=0: synchronous from the start.
    const bool kahan = kahan_mode(ctx) && ctx->ts.cs == QVQ_CS_SCALED;
    const bool multi = ctx->nranks > 1 && (ctx->comm || ctx->host_ar);
    static const bool spec_off = env_is("QVQ_SPECULATE", "0");
    bool spec = kahan && !spec_off;
    if (spec && (st = ensure_speculation(ctx, Kmax)) != QVQ_OK) return st;
    if (kahan && (st = ensure_apool(ctx, ctx->ts, 2)) != QVQ_OK) return st;
    // several ranks, speculative: one assignment buffer per level, so that every level's parent
    // assignment is still there when the deferred checks finish at the end of the call
    const uint32_t npool = spec && multi ? std::max<uint32_t>(4, bits + 1) : 4;
    if (spec && (st = ensure_apool(ctx, ctx->ts, npool)) != QVQ_OK) return st;
    ctx->kh.deferred.clear();
    struct JobGuard {   // no tree build or check outlives the call (an error return included)
        qvq_ctx *c;
        ~JobGuard() {
            join_tree_job(c, true);
            for (auto &v : c->ver) {
                v.cancel.store(true);
                join_verify(c, v);
            }
        }
    } job_guard{ctx};
    // distortion inputs, per-level counters and the codebook go to mapped pinned memory in one
    // launch (the mapped split-codebook buffer is free once the last tree is built); the copy's
    // own flag ends the wait: polling it wakes the host at once (a stream synchronize costs tens
    // of us of wake-up), and the wait is bounded (wait.hpp), so a peer rank that dies inside a
    // level's all-reduce ends this call with QVQ_ECOMM
    bool out_enqueued = false;
    uint64_t out_seq = 0;
    auto enqueue_out = [&]() -> qvq_status {
        if (ctx->timing_level == -1) HIPCHK(hipEventRecord(ctx->ev_end, ctx->stream));   // each record idles the GPU ~6 us
        uint8_t *dh_small = reinterpret_cast<uint8_t *>(ctx->h_ready.dev()) + 64;
        static_assert(3 * sizeof(double) + LEVEL_COUNTERS * sizeof(unsigned) <= 1024 - 64, "small results exceed the mapped area");
        const uint64_t cb_bytes = codebook ? (uint64_t)Kmax * ctx->ts.D * 8 : 0;
        uint64_t *done = reinterpret_cast<uint64_t *>(dh_small + (1024 - 64 - 8));
        out_seq = ++ctx->out_seq;
        HIPCHK(launch_copy_out(ctx->stream, ctx->d_dist_part, dh_small, 3 * sizeof(double), ctx->d_counters,
                               dh_small + 3 * sizeof(double), LEVEL_COUNTERS * sizeof(unsigned), ctx->lv.d_C64_cent, ctx->lv.h_cb.dev(),
                               cb_bytes, done, out_seq, ctx->d_counters + COPY_DONE_COUNTER));
        out_enqueued = true;
        return QVQ_OK;
    };
    // the published results out of the mapped buffers: distortion inputs, per-level counters,
    // the codebook (C4: 1.5 MB, ~60 us)
    double dres[3];
    unsigned stats[LEVEL_COUNTERS];
    bool results_copied = false;
    bool upd[32] = {};   // per level: a separate sums pass was timed (LevelSums::upd)
    auto copy_results = [&]() -> qvq_status {
        uint8_t *h_small = reinterpret_cast<uint8_t *>(ctx->h_ready.get()) + 64;
        const uint64_t cb_bytes = codebook ? (uint64_t)Kmax * ctx->ts.D * 8 : 0;
        qvq_status ws = wait_flag(ctx, reinterpret_cast<volatile uint64_t *>(h_small + (1024 - 64 - 8)), out_seq);
        if (ws != QVQ_OK) return ws;
        std::memcpy(dres, h_small, sizeof(dres));
        std::memcpy(stats, h_small + sizeof(dres), sizeof(stats));
        if (codebook) std::memcpy(codebook, ctx->lv.h_cb, cb_bytes);
        results_copied = true;
        ctx->htrace.mark("results copied");
        return QVQ_OK;
    };
    for (;;) {   // once, or twice when a speculative check fails
    out_enqueued = false;
    results_copied = false;
    const bool tmean = ctx->timing_level == -3;   // events around the mean kernel (qvq_set_timing)
    if (tmean) HIPCHK(hipEventRecord(ctx->ev[31][0], ctx->stream));
    HIPCHK(launch_mean_sums(ctx->stream, ctx->ts.Dp, ctx->ts.d_codes, ctx->ts.N, ctx->ts.D, ctx->d_plut, ctx->d_mean,
                            ctx->d_counters, N_COUNTERS, d_dist, hist, ctx->d_lut64));
    if (tmean) HIPCHK(hipEventRecord(ctx->ev[31][1], ctx->stream));
    if ((st = all_reduce_sums(ctx, 1, ctx->d_mean, MEAN_COPIES)) != QVQ_OK) {
        (void)hipMemsetAsync(ctx->d_mean, 0, MEAN_COPIES * (2 * 64 + 1) * 8, ctx->stream);   // keep it clear for the next call
        return st;
    }
    // finalize (+ split, tables, host codebook and its ready number) / final distortion
    // (K = 1 reads the mean sums and leaves them cleared for the next quantize)
    if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
    // the split a finalize writes: with deferred ties the level's own split must survive its
    // (speculative) finalize, so the next one goes to the other buffer and the two swap
    double *split_out = ctx->lv.d_C64_split;
    // The finalize of the K cells whose sums rs describes (K = 1: the mean sums), with the split
    // and the tables of the next level (its plan: next) or, at the last level (next null), the
    // distortion term.  clear1: the finalize also clears sums copy 1 after adding it (no fused
    // search of a later level clears it: a communicator, or the synchronous Kahan levels' moves).
    auto finalize = [&](uint32_t K, const LevelPlan *next, const ReducedSums &rs = ReducedSums(),
                        const TieExport &tx = TieExport(), bool clear1 = false) -> qvq_status {
        FinArgs f = finalize_args(ctx, K, true);
        sums_args(ctx, f, K == 1 ? nullptr : &rs, clear1);
        if (next) tables_args(ctx, f, 2, split_out, dev_cb_of(ctx, (uint32_t)__builtin_ctz(K) + 1), next->prunable);
        else f.dist_out = d_dist + 2;
        f.ties = tx;
        if (next || tx.out) ctx->seq++;
        else f.ready = nullptr;
        f.seq = ctx->seq;
        return run_finalize(ctx, f);
    };
    // the plan of the level about to run, made once, by the finalize's time before it
    LevelPlan plan = plan_level(ctx, 2);
    if ((st = finalize(1, bits > 0 ? &plan : nullptr)) != QVQ_OK) return st;
    // with bits >= 1 the first search writes every row's index
    if (bits == 0) HIPCHK(hipMemsetAsync(ctx->ts.d_A, 0, ctx->ts.N * 4, ctx->stream));

    const bool sync_kahan = kahan && !spec;
    if (sync_kahan) split_out = ctx->lv.d_C64_split_alt;
    // the assignment buffers (apool owns them; d_A, d_A_alt, d_A3 and d_A4 are views): level L
    // writes apool[L % P]; a check of level L reads A_{L-1} until level L + 3 starts (one rank) or
    // to the end of the call (several ranks, P > bits)
    const std::vector<DevBuf<uint32_t>> &abuf = ctx->ts.apool;
    const uint32_t P = spec ? (uint32_t)std::min<size_t>(abuf.size(), npool) : 4;
    std::vector<uint32_t *> alev(bits + 1, nullptr);   // A_L of this call
    bool spec_failed = false, local_fail = false;
    for (uint32_t lvl = 1; lvl <= bits; lvl++) {
        const uint32_t K = 1u << lvl;
        const int slot = (int)lvl - 1;
        if (spec) {
            if (lvl >= 4) {
                bool ok;
                ctx->htrace.mark("L" + std::to_string(lvl) + " joins check K" + std::to_string(ctx->ver[lvl % 3].K));
                if ((st = join_verify_bounded(ctx, ctx->ver[lvl % 3], ok)) != QVQ_OK) return st;
                ctx->htrace.mark("L" + std::to_string(lvl) + " joined");
                if (!ok && !multi) {
                    spec_failed = true;
                    break;
                }
                local_fail = local_fail || !ok;   // several ranks: every rank runs on to the vote
            }
            ctx->ts.d_A = abuf[lvl % P];
            ctx->ts.d_A_alt = abuf[(lvl + P - 1) % P];
            ctx->ts.d_A3 = abuf[(lvl + 1) % P];   // (P >= 4: the four views stay distinct across calls)
            ctx->ts.d_A4 = abuf[(lvl + 2) % P];
        } else if (kahan) {
            std::swap(ctx->ts.d_A, ctx->ts.d_A_alt);   // d_A_alt: the previous level's assignment
        }
        alev[lvl] = ctx->ts.d_A;
        const LevelPlan p = plan;
        const bool split = lvl < bits;
        if (split) plan = plan_level(ctx, 2 * K);
        const LevelPlan *next = split ? &plan : nullptr;
        LevelSums ls;
        if ((st = run_level(ctx, p, K, slot, true, host_cb_of(ctx, lvl), ctx->seq, sync_kahan, ls)) != QVQ_OK) return st;
        upd[slot] = ls.upd;
        if (spec) {   // the level's check: its tree now
            qvq_ctx::Verify &v = ctx->ver[lvl % 3];
            v.K = K;
            v.level = lvl;
            v.tree = std::move(ctx->tree);
            // (swapped, not moved: the joined check's buffers come back with their capacity, so
            // the next level's codebook copy writes no fresh pages -- 1.5 MB at C4's level 12)
            std::swap(v.cb, ctx->cb_local);
            std::swap(v.cnt, ctx->cnt_local);
            ctx->cb_local.clear();
            ctx->cnt_local.clear();
            v.cs = CertState();
        }
        {
            ReducedSums rs;
            if ((st = reduce_level(ctx, K, slot, ls, rs)) != QVQ_OK) return st;
            if ((st = all_reduce_sums(ctx, K)) != QVQ_OK) return st;
            TieExport tx;
            if (spec) {   // the level's tie rows and their indices go out with its codebook
                tx.rows = ctx->ts.d_ties;
                tx.cnt = ctx->d_counters + 2 * slot + 1;   // the level's ties
                tx.A = ctx->ts.d_A;
                tx.codes = ctx->ts.d_codes;
                tx.cap = ctx->tx_cap;
                tx.n_rows = ctx->ts.N;
                tx.out = ctx->h_tx[lvl % 3].dev();
            }
            if ((st = finalize(K, next, rs, tx)) != QVQ_OK) return st;
            if (spec) {   // the check of this level, on the worker
                qvq_ctx::Verify &v = ctx->ver[lvl % 3];
                v.posted = true;
                v.done.store(false);
                v.cancel.store(false);
                v.status = 1;
                v.seq = ctx->seq;
                v.par = (int)(lvl % 3);
                v.A_prev = lvl >= 2 ? ctx->ts.d_A_alt : nullptr;
                qvq_ctx::Verify *vp = &v;
                post_job(ctx, [ctx, vp] {
                    verify_level(ctx, *vp);
                    vp->done.store(true, std::memory_order_release);
                });
                ctx->htrace.mark("L" + std::to_string(lvl) + " finalize enqueued, check posted");
            }
            if (sync_kahan) {   // the level's ties (published after its recheck)
                if ((st = wait_flag(ctx, ctx->h_ready + 1, ctx->pub_seq)) != QVQ_OK) return st;
                const unsigned nt = (unsigned)(uint32_t)ctx->h_ready[2];
                uint64_t nt_all = nt;   // every rank's ties: the ranks resolve together
                if (multi && (st = vote(ctx, &nt_all, 1)) != QVQ_OK) return st;
                join_tree_job(ctx, nt_all == 0);   // the level's tree: needed for ties only
                if (nt_all) {   // the level's finalize again, over the sums with the ties' moves
                    // (several ranks: every rank's moves in copy 1, all-reduced, added by the finalize)
                    st = multi ? resolve_kahan_ties_multi(ctx, p, K, slot, nt, rs) : resolve_kahan_ties(ctx, p, K, slot, nt, rs);
                    if (st != QVQ_OK) return st;
                    // (a communicator: without kd_reduce no fused search clears copy 1 before its next use)
                    if ((st = finalize(K, next, rs, TieExport(), !kd_merge(ctx))) != QVQ_OK) return st;
                }
                if (split) {
                    std::swap(ctx->lv.d_C64_split, ctx->lv.d_C64_split_alt);
                    split_out = ctx->lv.d_C64_split_alt;
                }
            }
        }
    }
    if (spec && !spec_failed) {   // the results' copy overlaps the last checks
        if ((st = enqueue_out()) != QVQ_OK) return st;
        ctx->htrace.mark("results' copy enqueued");
        for (uint32_t l = bits >= 3 ? bits - 2 : 1; l <= bits; l++) {
            // one rank: the results leave the mapped buffers while the last check runs (a
            // failed check redoes the quantize, and the copy with it)
            if (l == bits && !multi && (st = copy_results()) != QVQ_OK) return st;
            bool ok;
            if ((st = join_verify_bounded(ctx, ctx->ver[l % 3], ok, true)) != QVQ_OK) return st;
            local_fail = local_fail || !ok;
        }
        ctx->htrace.mark("last checks joined");
        spec_failed = local_fail;
        if (multi && (st = resolve_deferred(ctx, bits, alev, spec_failed)) != QVQ_OK) return st;
    }
    ctx->kh.deferred.clear();
    if (!spec_failed) break;
    // a check failed: every check joined, the stream drained, then the quantize again with
    // synchronous Kahan levels
    for (auto &v : ctx->ver) {
        v.cancel.store(true);
        join_verify(ctx, v);
    }
    ctx->kh.deferred.clear();
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
    ctx->tm.kahan_redo++;
    spec = false;
    }
    // Returned distortion: updateDistortion after the last fix (src/Quantizer.cpp:9-22,103),
    // from the sums of the final assignment (finalize_kernel without tables).
    // (enqueue_out: before the last checks are joined when speculating)
    if (!out_enqueued && (st = enqueue_out()) != QVQ_OK) return st;
    if (!results_copied && (st = copy_results()) != QVQ_OK) return st;
    if (assign)   // every collective of this call is complete: a plain copy
        HIPCHK(host_copy(ctx, assign, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost));
    // closed form: sum ||x||^2 - sum_k (2 c_k.S_k - n_k ||c_k||^2) cancels to a few ulps of
    // sum ||x||^2 when the cells are (nearly) exact; a distortion is never negative
    const double dist_final = std::max(0.0, (dres[0] - dres[2]) / (dres[1] * (double)ctx->ts.D));
    if (distortion) *distortion = dist_final;
    lbg_timings(ctx, bits, upd, stats);
    (void)hipGetLastError();
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (htrace) {
        ctx->htrace.mark("return");
        std::fprintf(stderr, "%s\n", ctx->htrace.finish().c_str());
    }
    ctx->rf.valid = true;   // qvq_refine may continue from here
    ctx->rf.K = Kmax;
    ctx->rf.dist = dist_final;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_assign(qvq_ctx *ctx, const double *C, uint32_t K, uint32_t *assign) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (!C || K == 0) return fail(ctx, QVQ_EINVAL, "empty codebook");
    if (!ctx->ts.exact) {
        // the searches' near-tie thresholds (mfma_setup, valu_coeffs) and the f16 / fp32 score scale
        // 2^t hold for components in [cmin, cmax] only; NaN fails the comparison too
        double vmin, vmax, cmin, cmax;
        codebook_range(ctx->ts.terms, vmin, vmax, cmin, cmax);
        for (uint64_t i = 0; i < (uint64_t)K * ctx->ts.D; i++)
            if (!(C[i] >= cmin && C[i] <= cmax))
                return fail(ctx, QVQ_EINVAL, "codebook outside 1.2 times the colour space's value range");
    }
    ctx->rf.valid = false;
    HIPCHK(hipSetDevice(ctx->dev));
    qvq_status st = ensure_levels(ctx, K);
    if (st != QVQ_OK) return st;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    HIPCHK(hipMemcpy(ctx->lv.d_C64_split, C, (uint64_t)K * ctx->ts.D * 8, hipMemcpyHostToDevice));
    if (ctx->ts.exact) {
        unsigned nt = 0;
        if ((st = exact_assign(ctx, C, K, nt)) != QVQ_OK) return st;
        ctx->tm.levels = 1;
        ctx->tm.host_ties[0] = nt;
        if (assign) HIPCHK(hipMemcpy(assign, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost));
        return QVQ_OK;
    }
    HIPCHK(hipMemsetAsync(ctx->d_counters, 0, 2 * sizeof(unsigned), ctx->stream));
    if ((st = run_prep(ctx, K)) != QVQ_OK) return st;
    LevelSums ls;   // (no sums wanted)
    if ((st = run_level(ctx, plan_level(ctx, K), K, 0, false, C, 0, false, ls)) != QVQ_OK) return st;
    unsigned stats[2];
    HIPCHK(hipMemcpyAsync(stats, ctx->d_counters, sizeof(stats), hipMemcpyDeviceToHost, ctx->stream));
    if (assign) HIPCHK(hipMemcpyAsync(assign, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->tm.levels = 1;
    ctx->tm.flagged[0] = stats[0];
    ctx->tm.host_ties[0] = stats[1];
    return QVQ_OK;
}

QVQ_API qvq_status qvq_update(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, double *C_out, uint64_t *counts) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (!assign || K == 0) return fail(ctx, QVQ_EINVAL, "empty assignment");
    ctx->rf.valid = false;
    for (uint64_t i = 0; i < ctx->ts.N; i++)
        if (assign[i] >= K) return fail(ctx, QVQ_EINVAL, "assignment index out of range");
    HIPCHK(hipSetDevice(ctx->dev));
    qvq_status st = ensure_levels(ctx, K);
    if (st != QVQ_OK) return st;
    HIPCHK(hipMemcpy(ctx->ts.d_A, assign, ctx->ts.N * 4, hipMemcpyHostToDevice));
    if (ctx->ts.exact) {
        if ((st = exact_single_rank(ctx)) != QVQ_OK) return st;
        uint64_t *d_cnt = ctx->lv.d_sums;   // K u64 of scratch (2KD + K)
        if ((st = exact_centroids(ctx, false, K, d_cnt)) != QVQ_OK) return st;
        if (C_out) HIPCHK(hipMemcpyAsync(C_out, ctx->lv.d_C64_cent, (uint64_t)K * ctx->ts.D * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, d_cnt, (uint64_t)K * 8, hipMemcpyDeviceToHost, ctx->stream));
        return wait_stream(ctx);
    }
    if ((st = run_update(ctx, plan_level(ctx, K), ctx->ts.d_A, K)) != QVQ_OK) return st;
    if ((st = all_reduce_sums(ctx, K)) != QVQ_OK) return st;
    FinArgs f = finalize_args(ctx, K, false);   // the centroids only
    const ReducedSums rs;
    sums_args(ctx, f, &rs, false);
    if ((st = run_finalize(ctx, f)) != QVQ_OK) return st;
    // results land in context-owned pinned memory and reach the caller only after the bounded
    // wait succeeds (a failed wait can leave these copies queued: wait_failed)
    const uint64_t cB = (uint64_t)K * ctx->ts.D * 8, nB = (uint64_t)K * 8;
    HIPCHK(ctx->h_stage.ensure(cB + nB));
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    HIPCHK(hipMemcpyAsync(stage, ctx->lv.d_C64_cent, cB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + cB, ctx->lv.d_sums + 2 * (uint64_t)K * ctx->ts.D, nB, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;   // bounded: the all-reduce may wait on peer ranks
    if (C_out) std::memcpy(C_out, stage, cB);
    if (counts) std::memcpy(counts, stage + cB, nB);
    return QVQ_OK;
}

// The K Kahan centroids in d_kc_cent to the caller (C_out may be null): through context-owned
// pinned memory, which reaches the caller only after the bounded wait succeeds.
static qvq_status kahan_result(qvq_ctx *ctx, uint32_t K, double *C_out) {
    const uint64_t cB = (uint64_t)K * ctx->ts.D * 8;
    HIPCHK(ctx->h_stage.ensure(cB));
    HIPCHK(hipMemcpyAsync(ctx->h_stage, ctx->kh.cells.d_kc_cent, cB, hipMemcpyDeviceToHost, ctx->stream));
    const qvq_status st = wait_stream(ctx);
    if (st != QVQ_OK) return st;
    if (C_out) std::memcpy(C_out, ctx->h_stage, cB);
    return QVQ_OK;
}

// The reference's centroids bit for bit (Solution::fixCodeVectors, src/Quantizer.cpp:59-87):
// Kahan sums in ascending row order times fl(1/n) (k_kahan.hip).  One rank; byte rows.
QVQ_API qvq_status qvq_update_kahan(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, double *C_out) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (!assign || K == 0) return fail(ctx, QVQ_EINVAL, "empty assignment");
    ctx->rf.valid = false;
    if (ctx->ts.exact) return qvq_update(ctx, assign, K, C_out, nullptr);   // exact mode: the Kahan chain already
    if (ctx->ts.cs != QVQ_CS_SCALED) return qvq_update(ctx, assign, K, C_out, nullptr);   // integers: exact = Kahan
    for (uint64_t i = 0; i < ctx->ts.N; i++)
        if (assign[i] >= K) return fail(ctx, QVQ_EINVAL, "assignment index out of range");
    HIPCHK(hipSetDevice(ctx->dev));
    qvq_status st = ensure_levels(ctx, K);
    if (st != QVQ_OK) return st;
    if ((st = ensure_kahan(ctx, K)) != QVQ_OK) return st;
    HIPCHK(hipMemcpy(ctx->ts.d_A, assign, ctx->ts.N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(ctx->kh.kw.stats, 0, 4 * sizeof(unsigned), ctx->stream));   // this call's counters
    ctx->kh.last_route = QVQ_KAHAN_ROUTE_CHAINED;
    if (ctx->nranks > 1) {   // every rank's rows: the chains pass from rank to rank (kahan_chained)
        if ((st = kahan_chained(ctx, K == 1 ? nullptr : ctx->ts.d_A, K, nullptr, K, false)) != QVQ_OK)
            return st;
    } else {
        uint64_t max_rows = ctx->ts.N;   // the longest chain (short ones run step by step)
        if (K > 1) {
            std::vector<uint64_t> n(K, 0);
            for (uint64_t i = 0; i < ctx->ts.N; i++) n[assign[i]]++;   // (checked < K above)
            max_rows = std::max<uint64_t>(1, *std::max_element(n.begin(), n.end()));
        }
        ctx->kh.last_route = max_rows <= kahan_direct_max() ? QVQ_KAHAN_ROUTE_DIRECT : QVQ_KAHAN_ROUTE_FUNCTIONS;
        HIPCHK(launch_kahan_centroids(ctx->stream, ctx->kh.kw, ctx->ts.d_codes, ctx->ts.Dp, ctx->ts.D, ctx->ts.N,
                                      K == 1 ? nullptr : ctx->ts.d_A, K, ctx->kh.cells.d_kc_cent, nullptr, nullptr, 0, max_rows));
    }
    if ((st = kahan_result(ctx, K, C_out)) != QVQ_OK) return st;
    if (env_is("QVQ_KAHAN_DEBUG", "1")) {
        unsigned ms[4];
        HIPCHK(hipMemcpy(ms, ctx->kh.kw.stats, sizeof(ms), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "qvq kahan: K %u blocks not composable %u block misses %u replays %u\n", K, ms[0], ms[1],
                     ms[2]);
    }
    return QVQ_OK;
}

// Test entry: the route of the last qvq_update_kahan / qvq_update_kahan_split call and the
// counters its kernels kept (k_kahan.hip Geo::stats).
QVQ_API qvq_status qvq_get_kahan_stats(qvq_ctx *ctx, qvq_kahan_stats *out) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (!out) return fail(ctx, QVQ_EINVAL, "null output");
    if (!ctx->kh.last_route || !ctx->kh.kw.stats) return fail(ctx, QVQ_ESTATE, "no qvq_update_kahan has run");
    HIPCHK(hipSetDevice(ctx->dev));
    unsigned ms[4];
    HIPCHK(hipMemcpy(ms, ctx->kh.kw.stats, sizeof(ms), hipMemcpyDeviceToHost));
    out->route = ctx->kh.last_route;
    out->blocks_not_composable = ms[0];
    out->block_misses = ms[1];
    out->replays = ms[2];
    return QVQ_OK;
}

// Test entry: qvq_update_kahan with this context's rows cut into virtual ranks at splits[0..n]
// (0 = splits[0] <= ... <= splits[n] = N), the chained evaluation of several ranks run in turn on
// one device (kahan_chained).  The result must equal qvq_update_kahan's for any cuts.
QVQ_API qvq_status qvq_update_kahan_split(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, const uint64_t *splits,
                                          uint32_t nsplits, double *C_out) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (ctx->ts.exact || ctx->ts.cs != QVQ_CS_SCALED) return fail(ctx, QVQ_EUNSUPPORTED, "SCALED byte rows only");
    if (!assign || K == 0 || !splits || nsplits == 0) return fail(ctx, QVQ_EINVAL, "empty assignment or splits");
    ctx->rf.valid = false;
    if (splits[0] != 0 || splits[nsplits] != ctx->ts.N) return fail(ctx, QVQ_EINVAL, "splits must run from 0 to N");
    for (uint32_t i = 0; i < nsplits; i++)
        if (splits[i] > splits[i + 1]) return fail(ctx, QVQ_EINVAL, "splits must not decrease");
    for (uint64_t i = 0; i < ctx->ts.N; i++)
        if (assign[i] >= K) return fail(ctx, QVQ_EINVAL, "assignment index out of range");
    HIPCHK(hipSetDevice(ctx->dev));
    qvq_status st = ensure_levels(ctx, K);
    if (st != QVQ_OK) return st;
    HIPCHK(hipMemcpy(ctx->ts.d_A, assign, ctx->ts.N * 4, hipMemcpyHostToDevice));
    const std::vector<uint64_t> cuts(splits, splits + nsplits + 1);
    if ((st = ensure_kahan(ctx, K)) != QVQ_OK) return st;
    HIPCHK(hipMemsetAsync(ctx->kh.kw.stats, 0, 4 * sizeof(unsigned), ctx->stream));   // this call's counters
    ctx->kh.last_route = QVQ_KAHAN_ROUTE_CHAINED;
    if ((st = kahan_chained(ctx, K == 1 ? nullptr : ctx->ts.d_A, K, nullptr, K, false, &cuts)) != QVQ_OK)
        return st;
    return kahan_result(ctx, K, C_out);
}

// The distortion a finalize published through FinArgs::pub (h_ready + 4: [1] the term's bits), once
// the host has seen its ready number or drained the stream: the closed form sum ||x||^2 -
// sum_k (2 c_k.S_k - n_k ||c_k||^2) over the norm (rows * D), never negative.  The fence orders
// this and the caller's later reads of the page.
static double published_distortion(const qvq_ctx *ctx, double xsq, double norm) {
    std::atomic_thread_fence(std::memory_order_acquire);
    const volatile uint64_t *h_pub = ctx->h_ready + 4;
    const uint64_t bits = h_pub[1];
    double term;
    std::memcpy(&term, &bits, 8);
    return std::max(0.0, (xsq - term) / norm);
}

// sum ||x||^2 and the rows of D components, from a byte histogram on the host
static void hist_totals(const qvq_ctx *ctx, const uint64_t *hist, double &sq_out, uint64_t &rows_out) {
    long double sq = 0;
    uint64_t n = 0;
    for (int b = 0; b < 256; b++) {
        sq += (long double)hist[b] * (long double)ctx->ts.terms.v64[b] * (long double)ctx->ts.terms.v64[b];
        n += hist[b];
    }
    sq_out = (double)sq;
    rows_out = n / ctx->ts.D;
}

// One rank: sum ||x||^2 and the rows from the byte histogram, once per training set (rf.xsq, rf.rows).
static qvq_status ensure_xsq(qvq_ctx *ctx) {
    if (ctx->rf.have_xsq) return QVQ_OK;
    uint64_t hist[256], n;
    HIPCHK(hipMemcpy(hist, ctx->d_hist, sizeof(hist), hipMemcpyDeviceToHost));
    hist_totals(ctx, hist, ctx->rf.xsq, n);
    ctx->rf.rows = (double)n;
    ctx->rf.have_xsq = true;
    return QVQ_OK;
}

// Both iterations' level counters and the rows-changed total, cleared on the stream before a
// Lloyd run (an earlier run may have dropped a search).
static qvq_status clear_iteration_counters(qvq_ctx *ctx) {
    HIPCHK(hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(unsigned), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_counters + CHANGED_COUNTER, 0, 2 * sizeof(unsigned), ctx->stream));
    return QVQ_OK;
}

// Lloyd refinement at fixed K, resident on the device.  Iteration t + 1 is one
// run_level against C_t -- qvq_assign's searches, recheck and kd-tree ties, with the exact sums of
// the final assignment -- the reduce, the count of changed rows and the same-K finalize_kernel, which
// writes C_{t+1}, its search tables and tile order, and publishes C_{t+1}, the changed count and
// the distortion term to mapped memory.  The host waits once per iteration, inside run_level, for
// the codebook its tree build needs; the stop decision of iteration t comes with that codebook,
// after the search against C_t is enqueued.  A stop therefore leaves one search in flight: it is
// the FRESH assignment when that is wanted, and is drained and dropped otherwise.
// On a communicator the rows changed are counted into the u64 behind the level's
// sums and one all-reduce per iteration, between the reduce and the finalize, carries both: the
// codebook, the count and the distortion term -- all the stop rule reads -- are then the same on
// every rank.  Several ranks first exchange their verdicts on the call (the entry vote).
// One Lloyd run at K from the codebook in d_C64_cent: qvq_refine's loop as its contract words it
// (DESIGN.md 3.11), which qvq_refine runs once and qvq_lbg_lloyd once per level (3.15).  The
// caller has sized the buffers, cleared the iteration counters and the dirty sums, and holds
// sum ||x||^2 and the norm.
struct LloydRun {
    // in
    uint32_t K = 0, max_iters = 0;
    double eps = 0;
    bool fresh = false, reseed = false;
    bool cont = false;           // A_0 is in d_A and d0 its distortion
    bool tables_ready = false;   // C_0's tables, tile order and host copy (half 0) are enqueued already,
                                 // under ctx->seq (qvq_lbg_lloyd's split); else made here from d_C64_cent
    bool count_empty = false;    // every centroid step publishes its empty cells too (qvq_lbg_lloyd only)
    double d0 = 0, xsq = 0, norm = 0;
    uint64_t rows_all = 0;           // the rows of every rank
    uint64_t *changed64 = nullptr;   // a communicator: the changed total behind the level's sums
    ReseedWork rw;
    uint64_t *changed = nullptr;     // the caller's traces (max_iters entries, may be null)
    double *dist_trace = nullptr;
    std::vector<uint64_t> *reseeds = nullptr;   // the seeds placed per iteration, appended (may be null)
    // out
    uint32_t iters = 0;   // t: C_t is the codebook (host_cb_of(ctx, t)), the assignment is in d_A
    int stop = -1;
    double d_last = 0;
    uint64_t last_changed = 0, last_empty = 0, seeds = 0;   // the last iteration's; the seeds of all
};
static qvq_status lloyd_at_k(qvq_ctx *ctx, LloydRun &r) {
    const uint32_t K = r.K, max_iters = r.max_iters, D = ctx->ts.D;
    const bool fresh = r.fresh, reseed = r.reseed, cont = r.cont;
    const double eps = r.eps, d0 = r.d0, xsq = r.xsq, norm = r.norm;
    const uint64_t rows_all = r.rows_all;
    uint64_t *const changed64 = r.changed64, *const changed = r.changed;
    double *const dist_trace = r.dist_trace;
    const ReseedWork &rw = r.rw;
    qvq_status st;
    const LevelPlan plan = plan_level(ctx, K);   // every iteration's
    volatile uint64_t *h_pub = ctx->h_ready + 4;   // [4] rows changed, [5] the distortion term, [6] seeds placed, [7] empty cells
    // the empty cells of the sums a centroid step is about to take (before its finalize clears
    // their further copies and the gate)
    auto count_empty = [&](const ReducedSums &rs) -> qvq_status {
        if (r.count_empty)
            HIPCHK(launch_count_empty(ctx->stream, ctx->lv.d_sums, K, D, rs.copies, rs.copies > 1 ? sums_cap_stride(ctx) : 0,
                                      rs.gate, ctx->h_ready.dev() + 7));
        return QVQ_OK;
    };
    // C_t's tables, tile order and host copy (t = 0, rs null: from the starting codebook; else the
    // centroid step over the sums rs describes: copy 1, kd_reduce_kernel's moves, is added and then
    // cleared under its gate), or without tables the distortion term of C_t under those sums
    auto publish = [&](uint32_t t, bool tables, const ReducedSums *rs, unsigned *cnts, bool count) -> qvq_status {
        if (rs && tables && (st = count_empty(*rs)) != QVQ_OK) return st;
        FinArgs f = finalize_args(ctx, K, true);
        if (rs) sums_args(ctx, f, rs, true);
        f.C_src = ctx->lv.d_C64_cent;
        if (tables) tables_args(ctx, f, 1, ctx->lv.d_C64_split, dev_cb_of(ctx, t), plan.prunable);
        else f.measure = true;
        if (count && changed64) f.changed64 = changed64;
        else if (count) f.changed = ctx->d_counters + CHANGED_COUNTER;
        f.clear_cnt = cnts;
        f.pub = ctx->h_ready.dev() + 4;
        f.seq = ++ctx->seq;
        return run_finalize(ctx, f);
    };
    if (!r.tables_ready && (st = publish(0, true, nullptr, nullptr, false)) != QVQ_OK) return st;
    // QVQ_REFINE_RESEED: the centroid step in four parts.  The cells' rows and the number of empty
    // cells (before the finalize clears the sums' further copies and their gate); the centroids
    // C_{t+1} alone, with the changed count and the distortion term (which the seeds leave as they
    // are: an empty cell owns no row); the rows pass and the select, which seed C_{t+1} in place and
    // publish the seeds placed; the tables, tile order and host copy from the seeded codebook, the
    // form iteration 0 uses, which carries the ready number the host waits for.
    auto publish_reseeded = [&](uint32_t t, const ReducedSums &rs, unsigned *cnts, bool count) -> qvq_status {
        if ((st = count_empty(rs)) != QVQ_OK) return st;
        HIPCHK(launch_reseed_count(ctx->stream, ctx->lv.d_sums, K, D, rs.copies,
                                   rs.copies > 1 ? sums_cap_stride(ctx) : 0, rs.gate, rw));
        FinArgs f = finalize_args(ctx, K, true);
        sums_args(ctx, f, &rs, true);
        if (count) f.changed = ctx->d_counters + CHANGED_COUNTER;
        f.clear_cnt = cnts;
        f.pub = ctx->h_ready.dev() + 4;
        f.seq = ++ctx->seq;
        qvq_status s = run_finalize(ctx, f);
        if (s != QVQ_OK) return s;
        HIPCHK(launch_reseed_rows(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.N, ctx->ts.d_A, ctx->lv.d_C64_cent, K,
                                  ctx->d_lut64, ctx->ts.cs == QVQ_CS_SCALED, rw));
        HIPCHK(launch_reseed_select(ctx->stream, ctx->ts.d_codes, ctx->ts.Dp, D, ctx->ts.N, ctx->d_lut64, ctx->lv.d_C64_cent, K, rw,
                                    ctx->h_ready.dev() + 6));
        FinArgs g = finalize_args(ctx, K, true);
        g.C_src = ctx->lv.d_C64_cent;
        tables_args(ctx, g, 1, ctx->lv.d_C64_split, dev_cb_of(ctx, t), plan.prunable);
        g.seq = ++ctx->seq;
        return run_finalize(ctx, g);
    };

    uint32_t t = 0;        // iterations done: C_t is the codebook, A_t (t >= 1, or continuing) in d_A
    int stop = -1;
    bool have_A = cont, have_dprev = cont;
    double d_prev = d0, d_last = d0;
    // iteration t's published count and distortion, and the stop rule
    auto absorb = [&]() {
        const double d = published_distortion(ctx, xsq, norm);
        const uint64_t chg = (t == 1 && !cont) ? rows_all : h_pub[0];
        const uint64_t seeds = reseed ? h_pub[2] : 0;
        if (r.reseeds) r.reseeds->push_back(seeds);
        r.seeds += seeds;
        r.last_changed = chg;
        if (r.count_empty) r.last_empty = h_pub[3];
        if (changed) changed[t - 1] = chg;
        if (dist_trace) dist_trace[t - 1] = d;
        if (chg == 0 && seeds == 0) stop = QVQ_STOP_FIXED;
        else if (have_dprev && std::fabs(d_prev - d) / d_prev <= eps) stop = QVQ_STOP_EPS;
        else if (t == max_iters) stop = QVQ_STOP_MAXIT;
        d_prev = d_last = d;
        have_dprev = true;
    };
    for (;;) {
        if (t == max_iters && !fresh) {   // the last iteration's results; nothing else is in flight
            if ((st = wait_codebook(ctx, ctx->seq)) != QVQ_OK) return st;
            absorb();
            break;
        }
        const int slot = (int)(t & 1);
        if (have_A) std::swap(ctx->ts.d_A, ctx->ts.d_A_alt);   // d_A_alt: A_t; d_A takes the search against C_t
        LevelSums ls;   // (dropped with the search where the call stops without fresh)
        if ((st = run_level(ctx, plan, K, slot, true, host_cb_of(ctx, t), ctx->seq, false, ls)) != QVQ_OK) return st;
        if (t >= 1) absorb();   // (run_level waited for C_t)
        else if (max_iters == 0) stop = QVQ_STOP_MAXIT;
        // the sums of the assignment run_level just made, reduced into d_sums (a communicator:
        // run_level has answered the kd-tree ties itself, the sums are one copy and there is no gate)
        ReducedSums rs;
        if (stop >= 0) {
            if (fresh) {   // the search in flight is A* = assign(C_t): its sums, the distortion of (C_t, A*)
                if ((st = reduce_level(ctx, K, slot, ls, rs)) != QVQ_OK) return st;
                if ((st = all_reduce_sums(ctx, K)) != QVQ_OK) return st;   // every rank's rows of A*
                if ((st = publish(t, false, &rs, ctx->d_counters + 2 * slot, false)) != QVQ_OK) return st;
                if ((st = wait_codebook(ctx, ctx->seq)) != QVQ_OK) return st;
                std::atomic_thread_fence(std::memory_order_acquire);
                const uint64_t bits = h_pub[1];
                double term;
                std::memcpy(&term, &bits, 8);
                d_last = std::max(0.0, (xsq - term) / norm);
            } else {   // dropped: A_t stays the assignment
                if (have_A) std::swap(ctx->ts.d_A, ctx->ts.d_A_alt);
                if ((st = wait_stream(ctx)) != QVQ_OK) return st;
            }
            break;
        }
        if ((st = reduce_level(ctx, K, slot, ls, rs)) != QVQ_OK) return st;
        if (changed64) {   // the level's sums and the rows changed over every rank: one collective
            mark_sums1(ctx);   // (the slot lies in copy 1's range: cleared if the call ends before the finalize)
            if (have_A) HIPCHK(launch_count_changed64(ctx->stream, ctx->num_cu, ctx->ts.d_A, ctx->ts.d_A_alt, ctx->ts.N, changed64));
            if ((st = all_reduce(ctx, ctx->lv.d_sums, 2 * (uint64_t)K * D + K + 1, false)) != QVQ_OK) return st;
        } else if (have_A) {
            HIPCHK(launch_count_changed(ctx->stream, ctx->num_cu, ctx->ts.d_A, ctx->ts.d_A_alt, ctx->ts.N,
                                        ctx->d_counters + CHANGED_COUNTER));
        }
        if (reseed) st = publish_reseeded(t + 1, rs, ctx->d_counters + 2 * slot, have_A);
        else st = publish(t + 1, true, &rs, ctx->d_counters + 2 * slot, have_A || changed64);
        if (st != QVQ_OK) return st;
        have_A = true;
        t++;
    }
    r.iters = t;
    r.stop = stop;
    r.d_last = d_last;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_refine(qvq_ctx *ctx, uint32_t K, const double *C_start, uint32_t max_iters, double eps,
                              uint32_t flags, double *codebook, uint32_t *assign, double *distortion,
                              uint64_t *changed, double *dist_trace, qvq_refine_info *info) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    const bool fresh = (flags & QVQ_REFINE_FRESH) != 0;
    const bool reseed = (flags & QVQ_REFINE_RESEED) != 0;
    const bool cont = C_start == nullptr;
    const bool sharded = ctx->comm || ctx->host_ar;
    // this rank's own verdict on the call; with a communicator the ranks exchange it (below)
    // before any of them returns
    qvq_status lst = QVQ_OK;
    const char *lmsg = "";
    auto reject = [&](qvq_status s, const char *m) {
        lst = s;
        lmsg = m;
    };
    if (ctx->ts.N == 0) reject(QVQ_ESTATE, "no training set");
    else if (flags & ~(uint32_t)(QVQ_REFINE_FRESH | QVQ_REFINE_RESEED)) reject(QVQ_EINVAL, "unknown refine flags");
    else if (max_iters == 0 && !fresh) reject(QVQ_EINVAL, "max_iters = 0 needs QVQ_REFINE_FRESH");
    else if (K == 0 || K > (1u << 20)) reject(QVQ_EINVAL, "K must be in 1 .. 2^20");
    else if (!(eps >= 0)) reject(QVQ_EINVAL, "eps must be >= 0");
    else if (ctx->ts.exact) reject(QVQ_EUNSUPPORTED, "refinement of an exact-mode training set is not supported");
    else if (reseed && sharded) reject(QVQ_EUNSUPPORTED, "QVQ_REFINE_RESEED is not supported on a communicator");
    else if (reseed && ctx->ts.N >= 0xFFFFFFFFull) reject(QVQ_EUNSUPPORTED, "QVQ_REFINE_RESEED takes fewer than 2^32 - 1 rows");
    else if (cont) {
        if (!ctx->rf.valid) reject(QVQ_ESTATE, "no qvq_lbg or qvq_refine result to continue from");
        else if (ctx->rf.K != K) reject(QVQ_EINVAL, "K differs from the result to continue from");
    } else {
        double vmin, vmax, cmin, cmax;
        codebook_range(ctx->ts.terms, vmin, vmax, cmin, cmax);
        // (the searches' error bands assume |c| <= 1.2 vmax: valu_coeffs, mf_th)
        for (uint64_t i = 0; i < (uint64_t)K * ctx->ts.D; i++)
            if (!(C_start[i] >= vmin && C_start[i] <= vmax)) {
                reject(QVQ_EINVAL, "starting codebook outside the colour space's value range");
                break;
            }
    }
    if (sharded && ctx->nranks > 1) {
        // The entry vote: every rank's verdict and a digest of its arguments, one slot pair per
        // rank (the sum is then a gather: every rank sees the same table and decides alike).  No
        // rank goes on to a per-iteration collective that a peer will not join.
        uint64_t h = 0xcbf29ce484222325ull;   // FNV-1a
        auto mix = [&](const void *p, uint64_t n) {
            const uint8_t *b = static_cast<const uint8_t *>(p);
            for (uint64_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
        };
        uint64_t ebits;
        std::memcpy(&ebits, &eps, 8);
        const uint64_t head[5] = {K, max_iters, ebits, flags, cont ? 1u : 0u};
        mix(head, sizeof(head));
        if (!cont && K >= 1 && K <= (1u << 20)) mix(C_start, (uint64_t)K * ctx->ts.D * 8);
        const uint32_t R = (uint32_t)ctx->nranks;
        std::vector<uint64_t> v(2ull * R, 0);
        v[2 * ctx->rank] = lst == QVQ_OK ? 1 : 2;   // (0: the rank wrote nothing)
        v[2 * ctx->rank + 1] = h;
        HIPCHK(hipSetDevice(ctx->dev));
        qvq_status vs = vote(ctx, v.data(), v.size());
        if (vs != QVQ_OK) return vs;
        if (lst != QVQ_OK) return fail(ctx, lst, lmsg);
        for (uint32_t r = 0; r < R; r++)
            if (v[2 * r] != 1) return fail(ctx, QVQ_EINVAL, "a peer rank rejected the qvq_refine call");
        for (uint32_t r = 0; r < R; r++)
            if (v[2 * r + 1] != h)
                return fail(ctx, QVQ_EINVAL, "qvq_refine arguments differ between the ranks");
    }
    if (lst != QVQ_OK) return fail(ctx, lst, lmsg);
    const double d0 = ctx->rf.dist;
    ctx->rf.valid = false;
    ctx->rf.have_reseeds = true;
    ctx->rf.reseeds.clear();
    HIPCHK(hipSetDevice(ctx->dev));
    qvq_status st = ensure_levels(ctx, std::max<uint32_t>(K, 2));
    if (st != QVQ_OK) return st;
    if ((st = ensure_apool(ctx, ctx->ts, 2)) != QVQ_OK) return st;
    ReseedWork rw;
    if (reseed) {
        const uint64_t need = reseed_layout(K).total;
        HIPCHK(ctx->d_reseed.ensure(need));
        rw = reseed_work(ctx->d_reseed, K);
        HIPCHK(hipMemsetAsync(rw.state, 0, 16, ctx->stream));   // (an abandoned call may have left a count)
    }
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    const uint32_t D = ctx->ts.D;
    const uint64_t KD = (uint64_t)K * D;
    // sum ||x||^2 and the rows, from the byte histogram
    double xsq;
    uint64_t rows_all;   // the rows of every rank
    if (sharded) {   // of every rank's rows: the histogram all-reduced as integers, as qvq_lbg does (once per call)
        HIPCHK(hipMemcpyAsync(ctx->d_hist + 256, ctx->d_hist, 256 * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if ((st = all_reduce(ctx, ctx->d_hist + 256, 256, false)) != QVQ_OK) return st;
        HIPCHK(ctx->h_stage.ensure(256 * 8));
        HIPCHK(hipMemcpyAsync(ctx->h_stage, ctx->d_hist + 256, 256 * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((st = wait_stream(ctx)) != QVQ_OK) return st;   // bounded: the all-reduce may wait on peer ranks
        hist_totals(ctx, reinterpret_cast<const uint64_t *>(ctx->h_stage.get()), xsq, rows_all);
    } else {
        if ((st = ensure_xsq(ctx)) != QVQ_OK) return st;
        xsq = ctx->rf.xsq;
        rows_all = ctx->ts.N;
    }
    const double norm = (sharded ? (double)rows_all : ctx->rf.rows) * (double)D;
    // a communicator: the rows changed are counted into the u64 behind the level's sums and
    // all-reduced with them (one collective per iteration)
    const uint64_t cell_u64 = 2 * KD + K;
    uint64_t *const changed64 = sharded ? ctx->lv.d_sums + cell_u64 : nullptr;
    if (!cont) HIPCHK(hipMemcpy(ctx->lv.d_C64_cent, C_start, KD * 8, hipMemcpyHostToDevice));
    // both iterations' counters, the changed total; copy 1 of the sums if a quantize left it dirty
    if ((st = clear_iteration_counters(ctx)) != QVQ_OK) return st;
    if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
    if (changed64) HIPCHK(hipMemsetAsync(changed64, 0, 8, ctx->stream));
    LloydRun run;
    run.K = K;
    run.max_iters = max_iters;
    run.eps = eps;
    run.fresh = fresh;
    run.reseed = reseed;
    run.cont = cont;
    run.d0 = d0;
    run.xsq = xsq;
    run.norm = norm;
    run.rows_all = rows_all;
    run.changed64 = changed64;
    run.rw = rw;
    run.changed = changed;
    run.dist_trace = dist_trace;
    run.reseeds = &ctx->rf.reseeds;
    if ((st = lloyd_at_k(ctx, run)) != QVQ_OK) return st;
    const uint32_t t = run.iters;
    const int stop = run.stop;
    const double d_last = run.d_last;
    // C_t as the finalize published it (t = 0: the starting codebook's copy)
    if (codebook) std::memcpy(codebook, host_cb_of(ctx, t), KD * 8);
    if (assign) HIPCHK(host_copy(ctx, assign, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost));
    if (distortion) *distortion = d_last;
    if (info) {
        info->iters = t;
        info->stop = (uint32_t)stop;
    }
    (void)hipGetLastError();
    ctx->rf.valid = true;
    ctx->rf.K = K;
    ctx->rf.dist = d_last;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_get_refine_reseeds(qvq_ctx *ctx, uint64_t *out, uint32_t cap, uint32_t *iters) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (!ctx->rf.have_reseeds) return fail(ctx, QVQ_ESTATE, "no qvq_refine has run");
    if (cap && !out) return fail(ctx, QVQ_EINVAL, "null output");
    const uint32_t n = (uint32_t)ctx->rf.reseeds.size();
    for (uint32_t i = 0; i < std::min(n, cap); i++) out[i] = ctx->rf.reseeds[i];
    if (iters) *iters = n;
    return QVQ_OK;
}

// Split-LBG with Lloyd iterations at every level (the rule in qvq.h).  The mean as
// qvq_lbg forms it; then per level one finalize that writes the split of the codebook in
// d_C64_cent with the level's tables, tile order and host copy (level 1: from the mean's sums, the
// form qvq_lbg's first finalize has; later levels: from the codebook itself, which may hold
// seeds), and qvq_refine's loop from those tables (lloyd_at_k).  The buffers are sized once for
// 2^bits; no codebook crosses to the host and back between the levels.
QVQ_API qvq_status qvq_lbg_lloyd(qvq_ctx *ctx, uint32_t bits, uint32_t iters, double eps, uint32_t flags,
                                 double *codebook, uint32_t *assign, double *distortion, qvq_lloyd_level *levels) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    const bool reseed = (flags & QVQ_LLOYD_RESEED) != 0;
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (bits > 20) return fail(ctx, QVQ_EINVAL, "bits must be <= 20");
    if (iters == 0) return fail(ctx, QVQ_EINVAL, "iters must be >= 1");
    if (!(eps >= 0)) return fail(ctx, QVQ_EINVAL, "eps must be >= 0");
    if (flags & ~(uint32_t)QVQ_LLOYD_RESEED) return fail(ctx, QVQ_EINVAL, "unknown qvq_lbg_lloyd flags");
    if (ctx->ts.exact) return fail(ctx, QVQ_EUNSUPPORTED, "qvq_lbg_lloyd of an exact-mode training set is not supported");
    if (ctx->comm || ctx->host_ar) return fail(ctx, QVQ_EUNSUPPORTED, "qvq_lbg_lloyd is not supported on a communicator");
    if (reseed && ctx->ts.N >= 0xFFFFFFFFull) return fail(ctx, QVQ_EUNSUPPORTED, "QVQ_LLOYD_RESEED takes fewer than 2^32 - 1 rows");
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->dev));
    const uint32_t Kmax = 1u << bits, D = ctx->ts.D;
    qvq_status st = ensure_levels(ctx, std::max<uint32_t>(Kmax, 2));
    if (st != QVQ_OK) return st;
    if ((st = ensure_apool(ctx, ctx->ts, 2)) != QVQ_OK) return st;
    if (reseed) HIPCHK(ctx->d_reseed.ensure(reseed_layout(Kmax).total));
    if ((st = ensure_xsq(ctx)) != QVQ_OK) return st;
    const double xsq = ctx->rf.xsq, norm = ctx->rf.rows * (double)D;
    ctx->rf.valid = false;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
    // the mean's sums (the kernel also clears the level counters); the finalize that takes them
    // leaves them cleared for the next quantize
    HIPCHK(launch_mean_sums(ctx->stream, ctx->ts.Dp, ctx->ts.d_codes, ctx->ts.N, D, ctx->d_plut, ctx->d_mean, ctx->d_counters,
                            N_COUNTERS, ctx->d_dist_part, ctx->d_hist, ctx->d_lut64));
    std::vector<qvq_lloyd_level> lv(bits);
    double d_last = 0;
    uint32_t t_last = 0;   // the last level's iterations: its codebook is host_cb_of(ctx, t_last)
    if (bits == 0) {   // one cell: the mean and its distortion term, no tables
        FinArgs f = finalize_args(ctx, 1, true);
        sums_args(ctx, f, nullptr, false);
        f.pub = ctx->h_ready.dev() + 4;
        f.seq = ++ctx->seq;
        if ((st = run_finalize(ctx, f)) != QVQ_OK) return st;
        HIPCHK(hipMemsetAsync(ctx->ts.d_A, 0, ctx->ts.N * 4, ctx->stream));
        HIPCHK(ctx->h_stage.ensure((uint64_t)D * 8));
        HIPCHK(hipMemcpyAsync(ctx->h_stage, ctx->lv.d_C64_cent, (uint64_t)D * 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((st = wait_stream(ctx)) != QVQ_OK) return st;
        d_last = published_distortion(ctx, xsq, norm);
    }
    for (uint32_t l = 1; l <= bits; l++) {
        const uint32_t K = 1u << l, H = K / 2;
        // S = the split of C^(l-1), its tables, tile order and host copy
        FinArgs f = finalize_args(ctx, H, true);
        if (l == 1) sums_args(ctx, f, nullptr, false);
        else f.C_src = ctx->lv.d_C64_cent;
        tables_args(ctx, f, 2, ctx->lv.d_C64_split, dev_cb_of(ctx, 0), plan_level(ctx, K).prunable);
        f.seq = ++ctx->seq;
        if ((st = run_finalize(ctx, f)) != QVQ_OK) return st;
        // both iterations' counters and the changed total (the previous level may have dropped a search)
        if ((st = clear_iteration_counters(ctx)) != QVQ_OK) return st;
        LloydRun run;
        run.K = K;
        run.max_iters = iters;
        run.eps = eps;
        run.reseed = reseed;
        run.tables_ready = true;
        run.count_empty = true;
        run.xsq = xsq;
        run.norm = norm;
        run.rows_all = ctx->ts.N;
        if (reseed) {
            run.rw = reseed_work(ctx->d_reseed, K);
            HIPCHK(hipMemsetAsync(run.rw.state, 0, 16, ctx->stream));
        }
        if ((st = lloyd_at_k(ctx, run)) != QVQ_OK) return st;
        if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
        qvq_lloyd_level &o = lv[l - 1];
        o.iters = run.iters;
        o.stop = (uint32_t)run.stop;
        o.changed = run.last_changed;
        o.empty = run.last_empty;
        o.seeds = run.seeds;
        o.distortion = run.d_last;
        d_last = run.d_last;
        t_last = run.iters;
    }
    // every wait above was bounded and has succeeded: the outputs
    if (codebook) std::memcpy(codebook, bits ? (const void *)host_cb_of(ctx, t_last) : (const void *)ctx->h_stage.get(), (uint64_t)Kmax * D * 8);
    if (assign) HIPCHK(host_copy(ctx, assign, ctx->ts.d_A, ctx->ts.N * 4, hipMemcpyDeviceToHost));
    if (distortion) *distortion = d_last;
    if (levels)
        for (uint32_t l = 0; l < bits; l++) levels[l] = lv[l];
    (void)hipGetLastError();
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));   // (run_level's per-slot host times are the iterations', not levels')
    ctx->tm.levels = (int)bits;
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->rf.valid = true;   // qvq_refine may continue from here
    ctx->rf.K = Kmax;
    ctx->rf.dist = d_last;
    return QVQ_OK;
}

// Median cut on the device (the rule in qvq.h and median_cut_rule.hpp).  Per level
// two row passes over the code bytes (the ranges with the previous level's relabel, the histogram
// on the chosen axis) and two per-box launches (axis, cut); one more row pass applies the last
// level's cuts.  The centroids and the distortion term then come from the engine's exact sums:
// run_update and the same-K finalize without tables, the form qvq_refine's reseed step uses.  The
// labels live in d_A; nothing of qvq_lbg's state is touched but the buffers qvq_update uses too.
QVQ_API qvq_status qvq_median_cut(qvq_ctx *ctx, uint32_t bits, double *codebook, uint32_t *assign, double *distortion,
                                  uint32_t *cuts) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (bits > 20) return fail(ctx, QVQ_EINVAL, "bits must be <= 20");
    if (ctx->ts.exact) return fail(ctx, QVQ_EUNSUPPORTED, "median cut of an exact-mode training set is not supported");
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "median cut is not supported on a communicator (no min/max reduce)");
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->dev));
    const uint32_t K = 1u << bits, D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t N = ctx->ts.N, KD = (uint64_t)K * D;
    qvq_status st = ensure_levels(ctx, std::max<uint32_t>(K, 2));
    if (st != QVQ_OK) return st;
    if (ctx->mc.K < K || ctx->mc.D != D) {
        qvq_ctx::MedianCut mc;
        HIPCHK(mc.d_work.alloc(mc_layout(K, D).total));
        mc.K = K;
        mc.D = D;
        ctx->mc = std::move(mc);
    }
    const uint64_t cB = KD * 8, uB = 32 * sizeof(uint32_t);
    HIPCHK(ctx->h_stage.ensure(cB + uB));
    if ((st = ensure_xsq(ctx)) != QVQ_OK) return st;
    ctx->rf.valid = false;
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    ctx->tm.levels = (int)bits;
    if ((st = clear_dirty_sums(ctx)) != QVQ_OK) return st;
    const McWork w = mc_work(ctx->mc.d_work, ctx->mc.K, D);
    const bool timed = ctx->timing_level == -1;   // each record idles the GPU ~6 us
    uint32_t *const A = ctx->ts.d_A;
    HIPCHK(launch_mc_init(ctx->stream, D, w));
    for (uint32_t l = 1; l <= bits; l++) {
        const uint32_t half = 1u << (l - 1);
        if (timed) HIPCHK(hipEventRecord(ctx->ev[l - 1][0], ctx->stream));
        HIPCHK(launch_mc_rows(ctx->stream, ctx->ts.d_codes, Dp, D, N, A, half / 2, true, w));
        if (timed) HIPCHK(hipEventRecord(ctx->ev[l - 1][1], ctx->stream));
        HIPCHK(launch_mc_axis(ctx->stream, half, D, w));
        if (timed) HIPCHK(hipEventRecord(ctx->ev[l - 1][2], ctx->stream));
        HIPCHK(launch_mc_hist(ctx->stream, ctx->ts.d_codes, Dp, D, N, A, half, w));
        if (timed) HIPCHK(hipEventRecord(ctx->ev[l - 1][3], ctx->stream));
        HIPCHK(launch_mc_cut(ctx->stream, half, D, l, w));
    }
    HIPCHK(launch_mc_rows(ctx->stream, ctx->ts.d_codes, Dp, D, N, A, K / 2, false, w));
    if ((st = run_update(ctx, plan_level(ctx, K), A, K)) != QVQ_OK) return st;
    FinArgs f = finalize_args(ctx, K, true);   // the centroids and the distortion term, no tables
    const ReducedSums rs;
    sums_args(ctx, f, &rs, true);
    f.pub = ctx->h_ready.dev() + 4;
    f.seq = ++ctx->seq;
    if ((st = run_finalize(ctx, f)) != QVQ_OK) return st;
    if (timed) HIPCHK(hipEventRecord(ctx->ev_end, ctx->stream));
    // results land in context-owned pinned memory and reach the caller only after the bounded wait
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    HIPCHK(hipMemcpyAsync(stage, ctx->lv.d_C64_cent, cB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + cB, w.cuts, uB, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = wait_stream(ctx)) != QVQ_OK) return st;
    const double dist = published_distortion(ctx, ctx->rf.xsq, ctx->rf.rows * (double)D);
    if (codebook) std::memcpy(codebook, stage, cB);
    if (cuts && bits) std::memcpy(cuts, stage + cB, bits * sizeof(uint32_t));
    if (assign) HIPCHK(host_copy(ctx, assign, A, N * 4, hipMemcpyDeviceToHost));
    if (distortion) *distortion = dist;
    for (uint32_t l = 1; timed && l <= bits; l++) {
        float r = 0, h = 0, whole = 0;
        (void)hipEventSynchronize(ctx->ev_end);
        (void)hipEventElapsedTime(&r, ctx->ev[l - 1][0], ctx->ev[l - 1][1]);
        (void)hipEventElapsedTime(&h, ctx->ev[l - 1][2], ctx->ev[l - 1][3]);
        (void)hipEventElapsedTime(&whole, ctx->ev[l - 1][0], l < bits ? ctx->ev[l][0] : ctx->ev_end);
        ctx->tm.assign_ms[l - 1] = r + h;                          // the two row passes
        ctx->tm.other_ms[l - 1] = std::max(0.f, whole - r - h);    // axis, cut; the last level: relabel, sums, finalize
    }
    (void)hipGetLastError();
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return QVQ_OK;
}

// k-means++ seeding on the device (the rule in qvq.h, kmeanspp_rule.hpp).  The first
// seed is drawn here; then K - 1 rounds of select and update are queued on the stream with no host
// round trip, a last select publishes the final potential, and one bounded wait ends the call.
// Everything the call writes on the device is its own (ts.kpp): no resident state is touched.
QVQ_API qvq_status qvq_kmeanspp(qvq_ctx *ctx, uint32_t K, uint64_t seed, double *codebook, uint32_t *rows,
                                uint64_t *potential, qvq_kmeanspp_info *info) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    if (K == 0 || K > (1u << 20)) return fail(ctx, QVQ_EINVAL, "K must be in 1 .. 2^20");
    if (ctx->ts.exact) return fail(ctx, QVQ_EUNSUPPORTED, "k-means++ seeding of an exact-mode training set is not supported");
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "k-means++ seeding is not supported on a communicator (no prefix over ranks)");
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->dev));
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t N = ctx->ts.N;
    qvq_ctx::Training::KMeansPP &kp = ctx->ts.kpp;
    HIPCHK(kp.d_m.ensure(N));
    if (kp.K < K) {
        kp.K = 0;
        HIPCHK(kp.d_work.alloc(kmpp_layout(K, Dp).total));
        kp.K = K;
    }
    const KmppLayout lay = kmpp_layout(kp.K, Dp);
    const uint64_t pB = 8ull * K, rB = 4ull * K, cB = (uint64_t)K * Dp;   // staged: potential | rows | codes | state
    HIPCHK(ctx->h_stage.ensure(pB + rB + cB + 8));
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    const KmppWork w = kmpp_work(kp.d_work, kp.d_m, kp.K, Dp);
    const uint8_t *codes = ctx->ts.d_codes;
    HIPCHK(launch_kmpp_init(ctx->stream, codes, Dp, N, (uint32_t)kmpp_draw(seed, 0, N), K, w));
    HIPCHK(launch_kmpp_update(ctx->stream, codes, Dp, N, true, w));
    for (uint32_t j = 1; j < K; j++) {
        HIPCHK(launch_kmpp_select(ctx->stream, codes, Dp, N, j, K, seed, w));
        HIPCHK(launch_kmpp_update(ctx->stream, codes, Dp, N, false, w));
    }
    HIPCHK(launch_kmpp_select(ctx->stream, codes, Dp, N, K, K, seed, w));
    // results land in context-owned pinned memory and reach the caller only after the bounded wait
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    const uint8_t *base = kp.d_work;
    HIPCHK(hipMemcpyAsync(stage, base + lay.potential, pB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + pB, base + lay.rows, rB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + pB + rB, base + lay.seedcodes, cB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + pB + rB + cB, base, 8, hipMemcpyDeviceToHost, ctx->stream));
    qvq_status st = wait_stream(ctx);
    if (st != QVQ_OK) return st;
    uint32_t state[2];
    std::memcpy(state, stage + pB + rB + cB, 8);
    const uint32_t placed = state[1];
    if (potential) std::memcpy(potential, stage, pB);
    if (rows) std::memcpy(rows, stage + pB, rB);
    if (codebook) {   // a seed's values are its row's, as qvq_get_vectors gives them; past placed: the zero vector
        const uint8_t *sc = stage + pB + rB;
        for (uint32_t j = 0; j < K; j++)
            for (uint32_t d = 0; d < D; d++)
                codebook[(uint64_t)j * D + d] = j < placed ? ctx->ts.terms.v64[sc[(uint64_t)j * Dp + d]] : 0.0;
    }
    if (info) info->placed = placed;
    ctx->tm.levels = 0;
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return QVQ_OK;
}

// Greedy k-means++ seeding on the device (the rule in qvq.h, kmeanspp_rule.hpp): L trial
// rows a round, the one that lowers the potential most is kept.  The first seed is drawn here; then
// K - 1 rounds of select and evaluate are queued on the stream with no host round trip, a last select
// publishes round K - 1, and one bounded wait ends the call.  Everything the call writes on the
// device is its own (ts.kppg): no resident state is touched.
QVQ_API qvq_status qvq_kmeanspp_greedy(qvq_ctx *ctx, uint32_t K, uint64_t seed, uint32_t trials, double *codebook,
                                       uint32_t *rows, uint64_t *potential, uint32_t *trial, uint32_t *trial_rows,
                                       uint64_t *trial_potential, qvq_kmeanspp_greedy_info *info) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    uint32_t L = 0;
    if (!kmpp_greedy_trials(K, trials, &L)) return fail(ctx, QVQ_EINVAL, "K must be in 1 .. 2^20 and trials in 0 .. 16");
    if (ctx->ts.exact) return fail(ctx, QVQ_EUNSUPPORTED, "k-means++ seeding of an exact-mode training set is not supported");
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "k-means++ seeding is not supported on a communicator (no prefix over ranks)");
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->dev));
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t N = ctx->ts.N;
    qvq_ctx::Training::KMeansPPGreedy &kp = ctx->ts.kppg;
    const KmppgLayout lay = kmppg_layout(K, Dp);
    HIPCHK(kp.d_m.ensure(N));
    if (kp.work_bytes < lay.total) {
        kp.work_bytes = 0;
        HIPCHK(kp.d_work.alloc(lay.total));
        kp.work_bytes = lay.total;
    }
    // staged: potential | trial_potential | rows | trial | trial_rows | codes | state (the layout's order)
    const uint64_t pB = 8ull * K, tpB = trial_potential ? pB * KMPPG_MAX_TRIALS : 0, rB = 4ull * K,
                   trB = trial_rows ? rB * KMPPG_MAX_TRIALS : 0, cB = (uint64_t)K * Dp;
    const uint64_t oTP = pB, oR = oTP + tpB, oT = oR + rB, oTR = oT + rB, oC = oTR + trB, oS = oC + cB;
    HIPCHK(ctx->h_stage.ensure(oS + 8));
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    const KmppgWork w = kmppg_work(kp.d_work, kp.d_m, K, Dp);
    const uint8_t *codes = ctx->ts.d_codes;
    HIPCHK(launch_kmppg_init(ctx->stream, codes, Dp, N, (uint32_t)kmpp_draw(seed, 0, N), K, w));
    HIPCHK(launch_kmppg_evaluate(ctx->stream, codes, Dp, N, 0, L, w));
    for (uint32_t j = 1; j < K; j++) {
        HIPCHK(launch_kmppg_select(ctx->stream, codes, Dp, N, j, K, L, seed, w));
        HIPCHK(launch_kmppg_evaluate(ctx->stream, codes, Dp, N, j, L, w));
    }
    HIPCHK(launch_kmppg_select(ctx->stream, codes, Dp, N, K, K, L, seed, w));
    // results land in context-owned pinned memory and reach the caller only after the bounded wait
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    const uint8_t *base = kp.d_work;
    HIPCHK(hipMemcpyAsync(stage, base + lay.potential, pB, hipMemcpyDeviceToHost, ctx->stream));
    if (tpB) HIPCHK(hipMemcpyAsync(stage + oTP, base + lay.trial_potential, tpB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + oR, base + lay.rows, rB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + oT, base + lay.trial, rB, hipMemcpyDeviceToHost, ctx->stream));
    if (trB) HIPCHK(hipMemcpyAsync(stage + oTR, base + lay.trial_rows, trB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + oC, base + lay.seedcodes, cB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(stage + oS, base, 8, hipMemcpyDeviceToHost, ctx->stream));
    qvq_status st = wait_stream(ctx);
    if (st != QVQ_OK) return st;
    uint32_t state[2];
    std::memcpy(state, stage + oS, 8);
    const uint32_t placed = state[1];
    if (potential) std::memcpy(potential, stage, pB);
    if (trial_potential) std::memcpy(trial_potential, stage + oTP, tpB);
    if (rows) std::memcpy(rows, stage + oR, rB);
    if (trial) std::memcpy(trial, stage + oT, rB);
    if (trial_rows) std::memcpy(trial_rows, stage + oTR, trB);
    if (codebook) {   // a seed's values are its row's, as qvq_get_vectors gives them; past placed: the zero vector
        const uint8_t *sc = stage + oC;
        for (uint32_t j = 0; j < K; j++)
            for (uint32_t d = 0; d < D; d++)
                codebook[(uint64_t)j * D + d] = j < placed ? ctx->ts.terms.v64[sc[(uint64_t)j * Dp + d]] : 0.0;
    }
    if (info) info->placed = placed, info->trials = L;
    ctx->tm.levels = 0;
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return QVQ_OK;
}

// k-means|| seeding on the device (the rule in qvq.h, kmeans_par_rule.hpp).  Candidate 0
// is drawn here; the rounds (count, scan, scatter, update), the weights and the one-block reduction are
// queued on the stream with no host round trip, and one bounded wait ends the call.  Everything the
// call writes on the device is its own (ts.kpar): no resident state is touched.
QVQ_API qvq_status qvq_kmeans_par(qvq_ctx *ctx, uint32_t K, uint64_t seed, const qvq_kmeans_par_opts *opts,
                                  double *codebook, uint32_t *rows, uint32_t *cand_rows, uint64_t *cand_weights,
                                  qvq_kmeans_par_info *info) {
    if (!ctx) return QVQ_EINVAL;
    GUARD(ctx);
    if (ctx->ts.N == 0) return fail(ctx, QVQ_ESTATE, "no training set");
    KMeansParPlan p{};
    if (!kmeans_par_options(K, opts ? opts->rounds : 0, opts ? opts->ell : 0, opts ? opts->round_cap : 0, &p))
        return fail(ctx, QVQ_EINVAL,
                    "k-means||: K must be in 1 .. 2^16, rounds <= 16, ell <= 2^17, round_cap >= 1, 1 + rounds * round_cap <= 2^20");
    if (ctx->ts.exact) return fail(ctx, QVQ_EUNSUPPORTED, "k-means|| seeding of an exact-mode training set is not supported");
    if (ctx->comm || ctx->host_ar)
        return fail(ctx, QVQ_EUNSUPPORTED, "k-means|| seeding is not supported on a communicator (no sample over ranks)");
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->dev));
    const uint32_t D = ctx->ts.D, Dp = ctx->ts.Dp;
    const uint64_t N = ctx->ts.N;
    kmeans_par_shape(N, Dp, &p);
    qvq_ctx::Training::KMeansPar &kp = ctx->ts.kpar;
    const KmparLayout lay = kmpar_layout(K, Dp, p);
    HIPCHK(kp.d_m.ensure(N));
    HIPCHK(kp.d_near.ensure(N));
    HIPCHK(kp.d_mask.ensure((N + 63) / 64));
    HIPCHK(kp.d_work.ensure(lay.total));
    const uint64_t mc = p.max_candidates;
    const uint64_t sB = 256, crB = 4 * mc, cwB = 4 * mc, rB = 4ull * K, cB = (uint64_t)K * Dp;   // staged: state | cand_rows | cand_wt | rows | codes
    HIPCHK(ctx->h_stage.ensure(sB + crB + cwB + rB + cB));
    std::memset(&ctx->tm, 0, sizeof(ctx->tm));
    const KmparWork w = kmpar_work(kp.d_work, kp.d_m, kp.d_near, kp.d_mask, lay);
    const uint8_t *codes = ctx->ts.d_codes;
    const bool timed = ctx->timing_level == -3;   // events around the phases (qvq_set_timing)
    hipStream_t s = ctx->stream;
    if (timed) HIPCHK(hipEventRecord(ctx->ev[16][0], s));
    HIPCHK(launch_kmpar_init(s, codes, Dp, N, (uint32_t)kmpp_draw(seed, 0, N), K, p, lay, w));
    HIPCHK(launch_kmpar_update(s, codes, Dp, N, p, true, w));
    for (uint32_t r = 1; r <= p.rounds; r++) {
        if (timed) HIPCHK(hipEventRecord(ctx->ev[r - 1][0], s));
        HIPCHK(launch_kmpar_sample(s, codes, Dp, N, p, r, seed, w));
        if (timed) HIPCHK(hipEventRecord(ctx->ev[r - 1][1], s));
        HIPCHK(launch_kmpar_update(s, codes, Dp, N, p, false, w));
        if (timed) HIPCHK(hipEventRecord(ctx->ev[r - 1][2], s));
    }
    if (timed) HIPCHK(hipEventRecord(ctx->ev[16][1], s));
    HIPCHK(launch_kmpar_weights(s, codes, Dp, N, p, w));
    if (timed) HIPCHK(hipEventRecord(ctx->ev[16][2], s));
    HIPCHK(launch_kmpar_reduce(s, codes, Dp, N, p, K, seed, w));
    if (timed) HIPCHK(hipEventRecord(ctx->ev_end, s));
    // results land in context-owned pinned memory and reach the caller only after the bounded wait
    uint8_t *stage = static_cast<uint8_t *>(ctx->h_stage);
    const uint8_t *base = kp.d_work;
    HIPCHK(hipMemcpyAsync(stage, base, sB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(stage + sB, base + lay.cand_rows, crB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(stage + sB + crB, base + lay.cand_wt, cwB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(stage + sB + crB + cwB, base + lay.rows, rB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(stage + sB + crB + cwB + rB, base + lay.seedcodes, cB, hipMemcpyDeviceToHost, s));
    qvq_status st = wait_stream(ctx);
    if (st != QVQ_OK) return st;
    uint32_t state[24];
    std::memcpy(state, stage, sizeof(state));
    const uint32_t placed = state[6];
    if (cand_rows) std::memcpy(cand_rows, stage + sB, crB);
    if (cand_weights) {
        const uint32_t *wt = reinterpret_cast<const uint32_t *>(stage + sB + crB);
        for (uint64_t c = 0; c < mc; c++) cand_weights[c] = wt[c];
    }
    if (rows) std::memcpy(rows, stage + sB + crB + cwB, rB);
    if (codebook) {   // a seed's values are its row's, as qvq_get_vectors gives them; past placed: the zero vector
        const uint8_t *sc = stage + sB + crB + cwB + rB;
        for (uint32_t j = 0; j < K; j++)
            for (uint32_t d = 0; d < D; d++)
                codebook[(uint64_t)j * D + d] = j < placed ? ctx->ts.terms.v64[sc[(uint64_t)j * Dp + d]] : 0.0;
    }
    if (info) {
        info->placed = placed;
        info->candidates = state[1];
        info->rounds_run = state[4];
        info->truncated = state[5];
        std::memcpy(info->round_candidates, state + 8, sizeof(info->round_candidates));
        std::memcpy(info->potential, stage + 96, sizeof(info->potential));
    }
    if (timed) {   // other_ms[r - 1] round r's sample, assign_ms[r - 1] its update; update_ms[0] candidate 0's pass,
                   // update_ms[1] the weights, update_ms[2] the reduction
        float a = 0;
        (void)hipEventSynchronize(ctx->ev_end);
        for (uint32_t r = 1; r <= p.rounds; r++) {
            (void)hipEventElapsedTime(&a, ctx->ev[r - 1][0], ctx->ev[r - 1][1]);
            ctx->tm.other_ms[r - 1] = a;
            (void)hipEventElapsedTime(&a, ctx->ev[r - 1][1], ctx->ev[r - 1][2]);
            ctx->tm.assign_ms[r - 1] = a;
        }
        (void)hipEventElapsedTime(&a, ctx->ev[16][0], ctx->ev[0][0]);
        ctx->tm.update_ms[0] = a;
        (void)hipEventElapsedTime(&a, ctx->ev[16][1], ctx->ev[16][2]);
        ctx->tm.update_ms[1] = a;
        (void)hipEventElapsedTime(&a, ctx->ev[16][2], ctx->ev_end);
        ctx->tm.update_ms[2] = a;
        (void)hipGetLastError();
    }
    ctx->tm.levels = 0;
    ctx->tm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return QVQ_OK;
}

// ---------------------------------------------------------------------------------------
// Decode: CompressedImage::decompress (src/Compressor.cpp:156-165) as one device gather.
// ---------------------------------------------------------------------------------------
static qvq_status check_decode_args(qvq_ctx *ctx, uint32_t K, uint64_t nblocks, uint32_t xSize, uint32_t ySize,
                                    uint32_t bw, uint32_t bh) {
    if (!ctx) return QVQ_EINVAL;
    if (K == 0 || bw == 0 || bh == 0 || xSize == 0 || ySize == 0)
        return fail(ctx, QVQ_EINVAL, "decode: K, block and image sizes must be > 0");
    // the kernel's block-row count and wrap span are 32-bit
    if ((uint64_t)ySize + bh - 1 > 0xFFFFFFFFull || (uint64_t)xSize + bw - 1 > 0xFFFFFFFFull)
        return fail(ctx, QVQ_EINVAL, "decode: image size + block size - 1 exceeds 2^32 - 1");
    const uint64_t wB = ((uint64_t)xSize + bw - 1) / bw, hB = ((uint64_t)ySize + bh - 1) / bh;
    if (nblocks != wB * hB) return fail(ctx, QVQ_EINVAL, "decode: nblocks != ceil(x/bw)*ceil(y/bh)");
    if ((uint64_t)bw * bh * 3 > 0xFFFFFFFFull) return fail(ctx, QVQ_EINVAL, "decode: block too large");
    return QVQ_OK;
}

// One decode launch on stream s (0 = the legacy null stream, ordered after every blocking
// stream's work, as in the caller's own torch/HIP code) with the context's persistent
// out-of-range flag and signed-byte squared-error accumulator; orig (may be null) is the
// original raster for the raport's MSE.  Synchronises s.
static qvq_status run_decode(qvq_ctx *ctx, hipStream_t s, const uint8_t *d_cb, uint32_t K, const uint32_t *d_A,
                             uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh, uint8_t *d_rgb,
                             const uint8_t *d_orig, double *mse) {
    uint64_t *d_err = ctx->d_decode_stat;   // [0] squared error, [1] bad-index flag
    hipError_t e = hipMemsetAsync(d_err, 0, 16, s);
    if (e == hipSuccess)
        e = launch_decode(s, d_cb, K, bw * bh * 3, d_A, xSize, ySize, bw, bh, d_rgb, d_orig, d_err,
                          reinterpret_cast<uint32_t *>(d_err + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_decode_stat, d_err, 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, QVQ_EDEVICE, std::string("decode: ") + hipGetErrorString(e));
    if (ctx->h_decode_stat[1]) return fail(ctx, QVQ_EINVAL, "decode: code-vector index out of range");
    if (mse) *mse = (double)ctx->h_decode_stat[0] / ((double)xSize * ySize * 3);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_decode_device(qvq_ctx *ctx, const void *d_codebook, uint32_t K, const void *d_assign,
                                     uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                     void *d_rgb, void *stream) {
    qvq_status st = check_decode_args(ctx, K, nblocks, xSize, ySize, bw, bh);
    if (st != QVQ_OK) return st;
    GUARD(ctx);
    if (!d_codebook || !d_assign || !d_rgb) return fail(ctx, QVQ_EINVAL, "decode: null pointer");
    if ((uintptr_t)d_assign % 4) return fail(ctx, QVQ_EINVAL, "decode: assignment pointer not 4-byte aligned");
    HIPCHK(hipSetDevice(ctx->dev));
    // ordered after the engine's own queued work (e.g. the qvq_lbg that wrote d_assign) on
    // any stream the caller names, the legacy null stream included
    HIPCHK(hipEventRecord(ctx->ev_sync, ctx->stream));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, ctx->ev_sync, 0));
    return run_decode(ctx, (hipStream_t)stream, (const uint8_t *)d_codebook, K, (const uint32_t *)d_assign, xSize,
                      ySize, bw, bh, (uint8_t *)d_rgb, nullptr, nullptr);
}

QVQ_API qvq_status qvq_decode(qvq_ctx *ctx, const uint8_t *codebook, uint32_t K, const uint32_t *assign,
                              uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh, uint8_t *rgb) {
    return qvq_decode_mse(ctx, codebook, K, assign, nblocks, xSize, ySize, bw, bh, rgb, nullptr, nullptr);
}

QVQ_API qvq_status qvq_decode_mse(qvq_ctx *ctx, const uint8_t *codebook, uint32_t K, const uint32_t *assign,
                                  uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                  uint8_t *rgb, const uint8_t *orig, double *mse) {
    qvq_status st = check_decode_args(ctx, K, nblocks, xSize, ySize, bw, bh);
    if (st != QVQ_OK) return st;
    GUARD(ctx);
    if (!codebook || !assign || (!rgb && !mse) || (mse && !orig))
        return fail(ctx, QVQ_EINVAL, "decode: null pointer");
    HIPCHK(hipSetDevice(ctx->dev));
    // one scratch allocation, grown on demand and kept: codebook | indices | raster | original
    const uint64_t cbB = (uint64_t)K * bw * bh * 3, aB = nblocks * 4, rB = (uint64_t)xSize * ySize * 3;
    const uint64_t oA = (cbB + 15) & ~15ull, oR = (oA + aB + 15) & ~15ull, oO = (oR + rB + 15) & ~15ull;
    const uint64_t need = oO + (orig ? rB : 0);
    HIPCHK(ctx->d_decode.ensure(need));
    uint8_t *d = ctx->d_decode;
    HIPCHK(hipMemcpyAsync(d, codebook, cbB, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d + oA, assign, aB, hipMemcpyHostToDevice, ctx->stream));
    if (orig) HIPCHK(hipMemcpyAsync(d + oO, orig, rB, hipMemcpyHostToDevice, ctx->stream));
    st = run_decode(ctx, ctx->stream, d, K, reinterpret_cast<const uint32_t *>(d + oA), xSize, ySize, bw, bh, d + oR,
                    orig ? d + oO : nullptr, mse);
    if (st == QVQ_OK && rgb) {
        HIPCHK(hipMemcpyAsync(rgb, d + oR, rB, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return st;
}

QVQ_API qvq_status qvq_comm_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id size");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, QVQ_ECOMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id, &u, 128);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_comm_init(qvq_ctx *ctx, int nranks, int rank, const uint8_t id[128]) {
    GUARD(ctx);
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return QVQ_EINVAL;
    HIPCHK(hipSetDevice(ctx->dev));
    if (ctx->comm) {
        ncclCommDestroy(ctx->comm);
        ctx->comm = nullptr;
    }
    ctx->host_ar = nullptr;
    ctx->host_ar_user = nullptr;
    ctx->nranks = 1;
    ctx->rank = 0;
    // a communicator even for one rank: the caller asked for the collective path (it is
    // then a local copy per level, and the results equal the communicator-free run's)
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    NCCLCHK(ncclCommInitRank(&ctx->comm, nranks, u, rank));
    ctx->nranks = nranks;
    ctx->rank = rank;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_comm_init_host(qvq_ctx *ctx, int nranks, int rank, qvq_allreduce_fn fn, void *user) {
    GUARD(ctx);
    if (!fn || nranks < 1 || rank < 0 || rank >= nranks) return QVQ_EINVAL;
    if (ctx->comm) {
        HIPCHK(hipSetDevice(ctx->dev));
        ncclCommDestroy(ctx->comm);
        ctx->comm = nullptr;
    }
    ctx->host_ar = fn;
    ctx->host_ar_user = user;
    ctx->nranks = nranks;
    ctx->rank = rank;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_comm_info(const qvq_ctx *ctx, int *nranks, int *rank, int *kind) {
    if (!ctx) return QVQ_EINVAL;
    if (nranks) *nranks = ctx->nranks;
    if (rank) *rank = ctx->rank;
    if (kind) *kind = ctx->comm ? QVQ_COMM_RCCL : ctx->host_ar ? QVQ_COMM_HOST : QVQ_COMM_NONE;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_set_timeout(qvq_ctx *ctx, double seconds) {
    if (!ctx || !(seconds > 0)) return QVQ_EINVAL;
    ctx->timeout_s = seconds;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_set_timing(qvq_ctx *ctx, int level) {
    if (!ctx || level < -3 || level > 31) return QVQ_EINVAL;
    ctx->timing_level = level;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_get_timings(const qvq_ctx *ctx, qvq_timings *out) {
    if (!ctx || !out) return QVQ_EINVAL;
    *out = ctx->tm;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kdtree_nn(const double *C, uint32_t K, uint32_t dim, const double *Q, uint64_t nq,
                                      uint32_t *out) {
    if (!C || !Q || !out || K == 0 || dim == 0 || dim > 64) return QVQ_EINVAL;
    RefKDTree tree(C, K, (int)dim);
    for (uint64_t i = 0; i < nq; i++) out[i] = tree.nearest(Q + i * dim);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kdtree_image(const double *C, uint32_t K, uint32_t dim, void *img, uint64_t bytes,
                                         uint64_t *need) {
    if (!C || !need || K == 0 || dim == 0 || dim > 64) return QVQ_EINVAL;
    *need = kdb_host_layout(K, dim).total;
    if (!img || bytes < *need) return QVQ_EINVAL;
    RefKDTree tree(C, K, (int)dim);
    if (tree.num_nodes() > 2ull * K) return QVQ_EINVAL;   // (the layout holds 2K nodes)
    std::memset(img, 0, *need);
    tree.to_device_image(static_cast<uint8_t *>(img));
    return QVQ_OK;
}

QVQ_API qvq_status qvq_kdtree_device_check(qvq_ctx *ctx, const double *C, uint32_t K, uint32_t dim, double *build_ms,
                                           uint32_t *result) {
    if (!ctx || !C || !result || K == 0 || dim == 0 || dim > 64) return QVQ_EINVAL;
    GUARD(ctx);
    if (!kd_build_fits(K, dim)) return fail(ctx, QVQ_EUNSUPPORTED, "device kd build: K or dim too large");
    HIPCHK(hipSetDevice(ctx->dev));
    const KdbHostLayout L = kdb_host_layout(K, dim);
    DevBuf<double> dP, nbox, cbox;
    DevBuf<uint32_t> vind;
    DevBuf<KdbNode> nodes;
    DevBuf<uint8_t> flat;
    CoherentBuf<uint8_t> himg;
    Event e0, e1;
    HIPCHK(dP.alloc((uint64_t)K * dim));
    HIPCHK(nbox.alloc(2ull * K * 2 * dim));
    HIPCHK(cbox.alloc(2ull * K * 2 * dim));
    HIPCHK(vind.alloc(K));
    HIPCHK(nodes.alloc(2ull * K));
    HIPCHK(flat.alloc(tree_bytes(K, dim)));
    HIPCHK(himg.alloc(L.total));
    std::memset(himg, 0, sizeof(KdbHeader));
    HIPCHK(hipEventCreate(e0.put()));
    HIPCHK(hipEventCreate(e1.put()));
    HIPCHK(hipMemcpy(dP, C, (uint64_t)K * dim * 8, hipMemcpyHostToDevice));
    HIPCHK(hipEventRecord(e0, ctx->stream));
    HIPCHK(launch_kd_build(ctx->stream, dP, K, dim, vind, nodes, nbox, cbox, flat, himg.dev(), 1));
    HIPCHK(hipEventRecord(e1, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const KdbHeader &h = *reinterpret_cast<const KdbHeader *>(himg.get());
    if (build_ms) {   // the launch; phase 1, phase 2, the images (the kernel's 100 MHz stamps)
        build_ms[0] = ms;
        for (int i = 0; i < 3; i++) build_ms[1 + i] = (double)h.pad2[i] * 1e-5;
    }
    if (h.seq != 1 || h.status != 1) {
        *result = 2;   // the build gave up (capacity): the engine builds on the host then
        return QVQ_OK;
    }
    const RefKDTree dev(C, K, (int)dim, himg), host(C, K, (int)dim);
    std::string why;
    *result = host.same_as(dev, &why) ? 0u : 1u;
    if (*result) ctx->err = "device kd-tree differs: " + why;
    // the device image kd_resolve reads: the host flattening of the same tree, node ids aside
    std::vector<uint8_t> fimg(16ull * dim + (uint64_t)h.n_nodes * sizeof(KdNodeDev) + 4ull * K);
    HIPCHK(hipMemcpy(fimg.data(), flat, fimg.size(), hipMemcpyDeviceToHost));
    const double *flo = reinterpret_cast<const double *>(fimg.data());
    const KdNodeDev *fn = reinterpret_cast<const KdNodeDev *>(flo + 2 * dim);
    const uint32_t *fv = reinterpret_cast<const uint32_t *>(fn + h.n_nodes);
    const KdbNode *hn = reinterpret_cast<const KdbNode *>(himg + L.nodes);
    const uint32_t *hv = reinterpret_cast<const uint32_t *>(himg + L.vind);
    for (uint32_t i = 0; i < h.n_nodes && !*result; i++) {
        const KdNodeDev &a = fn[i];
        const KdbNode &b = hn[i];
        const bool leaf = b.child1 < 0;
        if (a.child1 != b.child1 || a.child2 != b.child2 || a.b != (int32_t)b.right ||
            a.a != (int32_t)(leaf ? b.left : ((uint32_t)b.divfeat | b.left << 8)) || (!leaf && (a.lo != b.divlow || a.hi != b.divhigh))) {
            *result = 1;
            ctx->err = "device kd_resolve image differs at node " + std::to_string(i);
        }
    }
    for (uint32_t i = 0; i < K && !*result; i++)
        if (fv[i] != hv[i]) {
            *result = 1;
            ctx->err = "device kd_resolve image vind differs";
        }
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_finalize(const uint64_t *hi, const uint64_t *lo, const uint64_t *cnt, uint32_t K,
                                     uint32_t dim, int colorspace, double *C_out) {
    Terms t;
    if (!hi || !lo || !cnt || !C_out) return QVQ_EINVAL;
    if (!make_terms(colorspace, t)) return QVQ_EUNSUPPORTED;
    for (uint64_t k = 0; k < K; k++)
        for (uint32_t d = 0; d < dim; d++)
            C_out[k * dim + d] = centroid_value(hi[k * dim + d], lo[k * dim + d], cnt[k], t.R, t.bias, t.scale);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_plan(uint32_t dim, uint32_t K, uint64_t n, qvq_plan *out) {
    if (!out || dim == 0 || K == 0 || n == 0) return QVQ_EINVAL;
    const uint32_t Dp = (dim + 3) & ~3u;
    if (Dp > 64) return QVQ_EINVAL;
    const LevelPlan lp = plan_level(dim, Dp, n, K);   // the plan run_level switches on, field by field
    qvq_plan p;
    std::memset(&p, 0, sizeof(p));
    p.search = lp.search;
    p.fused = lp.fusable;
    p.c32_staged = lp.c32_staged;
    p.cb_resident = lp.cb_resident;
    p.valu_tiles = lp.valu_tiles;
    p.prune = lp.prunable;
    p.recheck = lp.recheck;
    if (lp.sorted_sums) {
        p.update = QVQ_PLAN_UPDATE_SORTED;
    } else {
        p.update = lp.update.runs ? QVQ_PLAN_UPDATE_RUNS : QVQ_PLAN_UPDATE_LDS;
        p.update_copies = lp.update.runs ? lp.update.copies : lp.update.passes;
    }
    p.device_tree = !lp.kd_host && lp.tree_shape;
    *out = p;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_exact_plan(uint32_t dim, uint32_t K, qvq_exact_plan *out) {
    if (!out || dim == 0 || dim > 64 || K == 0) return QVQ_EINVAL;
    qvq_exact_plan p;
    p.kc = exact_chunk_codes(dim);
    p.chunks = (K + p.kc - 1) / p.kc;
    p.last_chunk = K - (p.chunks - 1) * p.kc;
    p.templated = exact_templated(dim) ? 1 : 0;
    p.tile_rows = exact_tile_rows(dim);
    *out = p;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_exact_grids(qvq_exact_grids *out) {
    if (!out) return QVQ_EINVAL;
    out->block = EX_THREADS;
    out->assign_blocks = EX_ASSIGN_GRID_CAP;
    out->iota_blocks = EX_IOTA_GRID_CAP;
    out->dist_blocks = EX_DIST_GRID_CAP;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_decode_plan(uint32_t K, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                        uint32_t align_flags, qvq_decode_plan *out) {
    // the shapes check_decode_args lets through
    if (!out || K == 0 || bw == 0 || bh == 0 || xSize == 0 || ySize == 0) return QVQ_EINVAL;
    if ((uint64_t)ySize + bh - 1 > 0xFFFFFFFFull || (uint64_t)xSize + bw - 1 > 0xFFFFFFFFull) return QVQ_EINVAL;
    if ((uint64_t)bw * bh * 3 > 0xFFFFFFFFull) return QVQ_EINVAL;
    static_assert(QVQ_DECODE_RASTER_UNALIGNED == DEC_RASTER_UNALIGNED && QVQ_DECODE_ORIG_UNALIGNED == DEC_ORIG_UNALIGNED &&
                      QVQ_DECODE_INDEX_UNALIGNED == DEC_INDEX_UNALIGNED && QVQ_DECODE_CODEBOOK_ODD == DEC_CODEBOOK_ODD &&
                      QVQ_DECODE_PIXELS == DEC_PIXELS && QVQ_DECODE_ROWS == DEC_ROWS && QVQ_DECODE_ROWS_H == DEC_ROWS_H,
                  "qvq.h's decode plan enumerators are decode_plan.hpp's");
    if (align_flags & ~15u) return QVQ_EINVAL;
    const DecodePlan dp = decode_plan(K, xSize, ySize, bw, bh, align_flags);   // the plan launch_decode switches on
    qvq_decode_plan p;
    std::memset(&p, 0, sizeof(p));
    p.kernel = dp.kernel;
    p.H = dp.H;
    p.lds = dp.lds;
    p.coal = dp.coal;
    p.grid = dp.grid;
    p.lds_bytes = dp.lds_bytes;
    p.rounds = dp.rounds;
    *out = p;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_ingest_grid(qvq_ingest_grid *out) {
    if (!out) return QVQ_EINVAL;
    out->block = ING_THREADS;
    out->blocks = ING_GRID_CAP;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_reseed_grid(qvq_reseed_grid *out) {
    if (!out) return QVQ_EINVAL;
    out->block = RSD_THREADS;
    out->blocks = RSD_GRID_CAP;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_row_error(const double *x, const double *c, uint32_t dim, int colorspace, uint32_t *q) {
    if (!x || !c || !q || dim == 0 || dim > 64) return QVQ_EINVAL;
    if (colorspace != QVQ_CS_NORMAL && colorspace != QVQ_CS_SCALED) return QVQ_EUNSUPPORTED;
    *q = reseed_row_error([&](uint32_t d) { return x[d]; }, c, dim, reseed_shift(colorspace == QVQ_CS_SCALED));
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_reseed_far_key(uint32_t q, uint32_t row, uint64_t *key) {
    if (!key) return QVQ_EINVAL;
    *key = reseed_far_key(q, row);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_reseed_select(const uint64_t *E, const uint64_t *n, const uint64_t *far, uint32_t K,
                                          uint32_t *empties_out, uint32_t *rows_out, uint32_t *m) {
    if (!E || !n || !far || !m || K == 0) return QVQ_EINVAL;
    std::vector<uint32_t> empties, donors;
    for (uint32_t k = 0; k < K; k++) {
        if (n[k] == 0) empties.push_back(k);
        if (reseed_is_donor(n[k], E[k])) donors.push_back(k);
    }
    std::sort(donors.begin(), donors.end(), [&](uint32_t a, uint32_t b) { return reseed_before(E[a], a, E[b], b); });
    const uint32_t cnt = (uint32_t)std::min(empties.size(), donors.size());
    for (uint32_t j = 0; j < cnt; j++) {
        if (empties_out) empties_out[j] = empties[j];
        if (rows_out) rows_out[j] = reseed_far_row(far[donors[j]]);
    }
    *m = cnt;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_median_cut_plan(uint32_t dim, uint32_t boxes, uint64_t n, qvq_median_cut_plan *out) {
    if (!out || dim == 0 || dim > 64 || boxes == 0 || boxes > (1u << 19) || (boxes & (boxes - 1)) || n == 0) return QVQ_EINVAL;
    const MedianCutPlan p = median_cut_plan(dim, boxes, n);
    out->range_lds = p.range_lds;
    out->hist_lds = p.hist_lds;
    out->full_hist = p.full_hist;
    out->block = p.block;
    out->range_cap = p.range_cap;
    out->hist_cap = p.hist_cap;
    out->range_grid = p.range_grid;
    out->hist_grid = p.hist_grid;
    out->lds_words = p.lds_words;
    out->range_groups = p.range_groups;
    out->hist_groups = p.hist_groups;
    out->range_group_boxes = p.range_group_boxes;
    out->hist_group_boxes = p.hist_group_boxes;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_median_cut_axis(const uint32_t *lo, const uint32_t *hi, uint32_t dim, uint32_t *axis) {
    if (!lo || !hi || !axis || dim == 0 || dim > 64) return QVQ_EINVAL;
    uint32_t range;
    *axis = mc_axis(lo, hi, dim, &range);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_median_cut_select(const uint32_t *hist, uint32_t lo, uint32_t hi, uint64_t n, uint32_t *t) {
    if (!hist || !t || lo >= hi || hi > 255) return QVQ_EINVAL;
    *t = mc_select(hist, lo, hi, n);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmpp_draw(uint64_t seed, uint64_t j, uint64_t T, uint64_t *t) {
    if (!t || T == 0) return QVQ_EINVAL;
    *t = kmpp_draw(seed, j, T);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmpp_weight(const uint8_t *codes_a, const uint8_t *codes_b, uint32_t Dp, uint32_t *w) {
    if (!codes_a || !codes_b || !w || Dp == 0 || Dp > 64 || (Dp & 3)) return QVQ_EINVAL;
    uint32_t a[16], b[16];
    std::memcpy(a, codes_a, Dp);
    std::memcpy(b, codes_b, Dp);
    const uint32_t nw = Dp / 4;
    for (uint32_t i = 0; i < nw; i++) a[i] = kmpp_ordinals(a[i]), b[i] = kmpp_ordinals(b[i]);
    *w = kmpp_weight(a, kmpp_norm(a, nw), b, kmpp_norm(b, nw), nw);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmeanspp_plan(uint64_t n, qvq_kmeanspp_plan *out) {
    if (!out || n == 0 || n > 0xFFFFFFFFull) return QVQ_EINVAL;
    const KMeansPPPlan p = kmeanspp_plan(n);
    out->block = p.block;
    out->segments = p.segments;
    out->seg_rows = p.seg_rows;
    out->segments_cap = KMPP_SEGMENTS_CAP;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmpp_trials(uint32_t K, uint32_t trials, uint32_t *L) {
    if (!L || !kmpp_greedy_trials(K, trials, L)) return QVQ_EINVAL;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmeans_par_join(uint64_t seed, uint32_t r, uint64_t row, uint64_t phi, uint32_t ell, uint32_t m,
                                            int *joins) {
    if (!joins || r == 0 || r > KMPAR_ROUNDS_MAX || ell > KMPAR_ELL_MAX || m >= (1u << 22)) return QVQ_EINVAL;
    *joins = kmpar_joins(kmpar_round_key(seed, r), row, phi, ell, m) ? 1 : 0;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kmeans_par_plan(uint64_t n, uint32_t dim, uint32_t K, const qvq_kmeans_par_opts *opts,
                                            qvq_kmeans_par_plan *out) {
    if (!out || n == 0 || n > 0xFFFFFFFFull || dim == 0 || dim > 64) return QVQ_EINVAL;
    KMeansParPlan p{};
    if (!kmeans_par_options(K, opts ? opts->rounds : 0, opts ? opts->ell : 0, opts ? opts->round_cap : 0, &p)) return QVQ_EINVAL;
    kmeans_par_shape(n, (dim + 3) & ~3u, &p);
    out->rounds = p.rounds, out->ell = p.ell, out->round_cap = p.round_cap;
    out->block = p.block, out->segments = p.segments, out->seg_rows = p.seg_rows, out->segments_cap = KMPP_SEGMENTS_CAP;
    out->chunk = p.chunk, out->max_candidates = p.max_candidates;
    out->reduce_block = KMPAR_RED_THREADS, out->gw_lds = p.gw_lds, out->codes_lds = p.codes_lds, out->lds_bytes = p.lds_bytes;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_mean_grid(uint64_t n, uint32_t dim, qvq_mean_grid *out) {
    if (!out || n == 0 || n > 0xFFFFFFFFull || dim == 0 || dim > 64) return QVQ_EINVAL;
    const MeanPlan p = mean_plan(n, (dim + 3) & ~3u);   // the plan launch_mean_sums launches
    out->blocks = (uint32_t)p.grid;
    out->block = p.threads;
    out->group_rows = p.group_rows;
    out->chunk_groups = p.chunk_groups;
    out->chunks_in_flight = p.chunks_in_flight;
    out->groups_in_flight = p.groups_in_flight;
    out->chunk_loop = p.chunk_loop;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_kahan_sort_plan(uint32_t K, qvq_kahan_sort_plan *out) {
    if (!out || K == 0) return QVQ_EINVAL;
    out->window_keys = KahanWork::sort_window_keys();
    out->windows = KahanWork::sort_windows(K);
    out->lds_bytes = std::min(K, out->window_keys) * 4;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_tile64_grid(qvq_tile64_grid *out) {
    if (!out) return QVQ_EINVAL;
    out->block = T64_THREADS;
    out->blocks = T64_GRID_CAP;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_cie1931(const uint8_t *rgb, uint64_t npix, double *out) {
    if (!rgb || !out) return QVQ_EINVAL;
    for (uint64_t i = 0; i < npix; i++)
        cie1931_from_rgb((signed char)rgb[3 * i], (signed char)rgb[3 * i + 1], (signed char)rgb[3 * i + 2], out + 3 * i);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_colorspace_values(int colorspace, double out[256]) {
    Terms t;
    if (!out) return QVQ_EINVAL;
    if (!make_terms(colorspace, t)) return QVQ_EUNSUPPORTED;
    std::memcpy(out, t.v64, sizeof(t.v64));
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_classify(const double *X, uint64_t n, uint32_t dim, int32_t *colorspace, uint8_t *codes) {
    if (!X || !colorspace || n == 0 || dim == 0 || dim > 64) return QVQ_EINVAL;
    *colorspace = host_classify(X, n, dim, codes, nullptr);
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_wait_probe(int scenario, double timeout_s, double *elapsed_s) {
    if (scenario < 0 || scenario > 5 || !(timeout_s > 0)) return QVQ_EINVAL;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    auto after = [&](double s) { return std::chrono::duration<double>(clock::now() - t0).count() >= s; };
    std::string err;
    const qvq_status st = wait_until(
        [&] { return scenario == 0 && after(0.005); },
        [&](std::string &m) {
            if (scenario == 4) {
                m = "scripted stream fault";
                return StreamState::Failed;
            }
            return scenario == 5 ? StreamState::Drained : StreamState::Running;
        },
        [&](std::string &m) {
            if (scenario == 3 && after(0.005)) {
                m = "scripted peer failure";
                return CommState::Failed;
            }
            return scenario == 2 || scenario == 3 ? CommState::Healthy : CommState::None;
        },
        timeout_s, err);
    if (elapsed_s) *elapsed_s = std::chrono::duration<double>(clock::now() - t0).count();
    if (st != QVQ_OK) g_static_err = err;
    return st;
}

QVQ_API qvq_status qvq_host_pool_stress(uint32_t rounds, uint32_t maxn, uint64_t *errors) {
    if (!errors || maxn < 1 || maxn > 64) return QVQ_EINVAL;
    std::unique_ptr<qvq_ctx> ctx(new qvq_ctx());   // the pool only: no device work
    std::atomic<uint32_t> hits[64];
    uint64_t bad = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        // n grows and shrinks (new helpers spawn while earlier epochs exist, idle ones wake late)
        const uint32_t n = 1 + (uint32_t)(((uint64_t)r * 2654435761u) >> 7) % maxn;
        for (auto &h : hits) h.store(0);
        pool_run(ctx.get(), n, [&](uint32_t t) {
            hits[t].fetch_add(1);
            if ((t + r) % 5 == 0) std::this_thread::yield();
        });
        for (uint32_t t = 0; t < 64; t++) bad += hits[t].load() != (t < n ? 1u : 0u);
    }
    {
        std::lock_guard<std::mutex> g(ctx->pool.m);
        ctx->pool.stop.store(true);
    }
    ctx->pool.cv.notify_all();
    for (auto &t : ctx->pool.th) t.join();
    *errors = bad;
    return QVQ_OK;
}

QVQ_API qvq_status qvq_host_row_terms(const uint8_t *codes, uint32_t dim, int colorspace, uint64_t *hi,
                                      uint64_t *lo) {
    Terms t;
    if (!codes || !hi || !lo) return QVQ_EINVAL;
    if (!make_terms(colorspace, t)) return QVQ_EUNSUPPORTED;
    for (uint32_t d = 0; d < dim; d++) {
        hi[d] = t.hi[codes[d]];
        lo[d] = t.lo[codes[d]];
    }
    return QVQ_OK;
}

}  // extern "C"
