"""quant_amd -- MI355X LBG vector-quantization engine (Python mirror of the C ABI).

The product is libqvq.so (quant_amd/lib), a C-ABI library of hand-written HIP kernels
for gfx950 (include/qvq.h).  This module binds it with ctypes and mirrors the
reference's quantizer plugin interface (include/Quantizer.hpp:8-20):

    getQuantizer(Quantizers.LBG).quantize(trainingSet, n, eps) -> (codebook, assigned, distortion)

There is no CPU fallback: every compute call goes to the GPU through libqvq.so and raises
QVQError when the library or the device is missing.
"""
import ctypes
import sys
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QVQ_LIB") or os.path.join(_HERE, "lib", "libqvq.so")   # QVQ_LIB: A/B builds (tools/)

NORMAL, SCALED, CIE1931 = 0, 1, 2   # enum class ColorSpaces (include/ColorSpace.hpp:6)


class QVQError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("qvq status %d: %s" % (status, msg))
        self.status = status


class _Timings(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_int), ("total_ms", ctypes.c_double),
                ("assign_ms", ctypes.c_double * 32), ("update_ms", ctypes.c_double * 32),
                ("other_ms", ctypes.c_double * 32), ("flagged", ctypes.c_uint64 * 32),
                ("host_ties", ctypes.c_uint64 * 32), ("wait_ms", ctypes.c_double * 32),
                ("tree_ms", ctypes.c_double * 32), ("kahan_redo", ctypes.c_int), ("tie_overflow", ctypes.c_int),
                ("kahan_relays", ctypes.c_int), ("mean_ms", ctypes.c_double)]


class _Plan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("search", "fused", "c32_staged", "cb_resident", "valu_tiles",
                                                "recheck", "update", "update_copies", "prune", "device_tree")]


class _ExactPlan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("kc", "chunks", "last_chunk", "templated", "tile_rows")]


class _DecodePlan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("kernel", "H", "lds", "coal", "grid", "lds_bytes")] + \
               [("rounds", ctypes.c_uint64)]


class _ExactGrids(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("block", "assign_blocks", "iota_blocks", "dist_blocks")]


class _TrainingInfo(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_uint32), ("colorspace", ctypes.c_int32), ("n", ctypes.c_uint64),
                ("dim", ctypes.c_uint32)]


class _IngestGrid(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("block", "blocks")]


class _MedianCutPlan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("range_lds", "hist_lds", "full_hist", "block", "range_cap",
                                                "hist_cap", "range_grid", "hist_grid", "lds_words", "range_groups",
                                                "hist_groups", "range_group_boxes", "hist_group_boxes")]


class _KMeansPPPlan(ctypes.Structure):   # qvq_kmeanspp_plan
    _fields_ = [(f, ctypes.c_uint32) for f in ("block", "segments", "seg_rows", "segments_cap")]


class _KMeansPPGreedyInfo(ctypes.Structure):   # qvq_kmeanspp_greedy_info
    _fields_ = [("placed", ctypes.c_uint32), ("trials", ctypes.c_uint32)]


class _KMeansParOpts(ctypes.Structure):   # qvq_kmeans_par_opts
    _fields_ = [(f, ctypes.c_uint32) for f in ("rounds", "ell", "round_cap")]


class _KMeansParInfo(ctypes.Structure):   # qvq_kmeans_par_info
    _fields_ = [("placed", ctypes.c_uint32), ("candidates", ctypes.c_uint32), ("rounds_run", ctypes.c_uint32),
                ("truncated", ctypes.c_uint32), ("round_candidates", ctypes.c_uint32 * 16),
                ("potential", ctypes.c_uint64 * 17)]


class _KMeansParPlan(ctypes.Structure):   # qvq_kmeans_par_plan
    _fields_ = [(f, ctypes.c_uint32) for f in ("rounds", "ell", "round_cap", "block", "segments", "seg_rows",
                                                "segments_cap", "chunk", "max_candidates", "reduce_block", "gw_lds",
                                                "codes_lds", "lds_bytes")]


class _MeanGrid(ctypes.Structure):   # qvq_mean_grid
    _fields_ = [(f, ctypes.c_uint32) for f in ("blocks", "block", "group_rows", "chunk_groups", "chunks_in_flight",
                                                "groups_in_flight", "chunk_loop")]


class _KahanSortPlan(ctypes.Structure):   # qvq_kahan_sort_plan
    _fields_ = [(f, ctypes.c_uint32) for f in ("window_keys", "windows", "lds_bytes")]


class _KahanStats(ctypes.Structure):   # qvq_kahan_stats
    _fields_ = [(f, ctypes.c_uint32) for f in ("route", "blocks_not_composable", "block_misses", "replays")]


class _LloydLevel(ctypes.Structure):   # qvq_lloyd_level
    _fields_ = [("iters", ctypes.c_uint32), ("stop", ctypes.c_uint32), ("changed", ctypes.c_uint64),
                ("empty", ctypes.c_uint64), ("seeds", ctypes.c_uint64), ("distortion", ctypes.c_double)]


# qvq_plan enumerators (qvq.h)
PLAN_SEARCH_SMALL, PLAN_SEARCH_MF32, PLAN_SEARCH_WIDE, PLAN_SEARCH_VALU = 0, 1, 2, 3
PLAN_RECHECK_MF32, PLAN_RECHECK_STAGED, PLAN_RECHECK_CHUNKED, PLAN_RECHECK_GLOBAL = 0, 1, 2, 3
PLAN_UPDATE_RUNS, PLAN_UPDATE_SORTED, PLAN_UPDATE_LDS = 0, 1, 2
# qvq_decode_plan enumerators and qvq_host_decode_plan's align_flags (qvq.h)
DECODE_PIXELS, DECODE_ROWS, DECODE_ROWS_H = 0, 1, 2
DECODE_RASTER_UNALIGNED, DECODE_ORIG_UNALIGNED, DECODE_INDEX_UNALIGNED, DECODE_CODEBOOK_ODD = 1, 2, 4, 8
# qvq_kahan_stats.route (qvq.h)
KAHAN_ROUTE_DIRECT, KAHAN_ROUTE_FUNCTIONS, KAHAN_ROUTE_CHAINED = 1, 2, 3

_lib = None
EXPORTED = ["qvq_create", "qvq_destroy", "qvq_last_error", "qvq_version", "qvq_set_images",
            "qvq_set_images_device", "qvq_set_synthetic", "qvq_set_vectors", "qvq_num_vectors",
            "qvq_dim", "qvq_lbg", "qvq_assign_device", "qvq_assign", "qvq_update", "qvq_update_kahan",
            "qvq_comm_unique_id", "qvq_comm_init", "qvq_set_timing", "qvq_get_timings", "qvq_host_kdtree_nn",
            "qvq_host_finalize", "qvq_host_row_terms", "qvq_decode", "qvq_decode_mse", "qvq_decode_device",
            "qvq_set_timeout", "qvq_host_wait_probe", "qvq_comm_init_host", "qvq_comm_info", "qvq_set_vectors_exact",
            "qvq_update_kahan_split", "qvq_host_pool_stress", "qvq_kdtree_device_check",
            "qvq_host_kdtree_image", "qvq_refine", "qvq_host_plan", "qvq_host_exact_plan",
            "qvq_host_exact_grids", "qvq_set_vectors_device", "qvq_get_training_info", "qvq_get_ingest_ms",
            "qvq_host_colorspace_values", "qvq_host_classify", "qvq_host_ingest_grid", "qvq_get_vectors",
            "qvq_host_cie1931", "qvq_host_tile64_grid", "qvq_get_refine_reseeds", "qvq_host_row_error",
            "qvq_host_reseed_far_key", "qvq_host_reseed_select", "qvq_host_reseed_grid", "qvq_host_decode_plan",
            "qvq_median_cut", "qvq_host_median_cut_plan", "qvq_host_median_cut_axis",
            "qvq_host_median_cut_select", "qvq_lbg_lloyd", "qvq_kmeanspp", "qvq_host_kmpp_draw",
            "qvq_host_kmpp_weight", "qvq_host_kmeanspp_plan", "qvq_get_kahan_stats", "qvq_host_kahan_sort_plan",
            "qvq_host_mean_grid", "qvq_kmeans_par", "qvq_host_kmeans_par_join", "qvq_host_kmeans_par_plan",
            "qvq_kmeanspp_greedy", "qvq_host_kmpp_trials"]

COMM_NONE, COMM_RCCL, COMM_HOST = 0, 1, 2
REFINE_FRESH, REFINE_RESEED = 1, 2            # qvq_refine flags
LLOYD_RESEED = 1                              # qvq_lbg_lloyd flags
VECTORS_EXACT = 1                             # qvq_set_vectors_device flags
MODE_NONE, MODE_BYTE, MODE_EXACT = 0, 1, 2    # qvq_training_info.mode
STOP_FIXED, STOP_EPS, STOP_MAXIT = 0, 1, 2    # qvq_refine_info.stop
# int fn(void *buf, uint64_t count, int dtype, void *user) (qvq.h, qvq_comm_init_host)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p)


def lib():
    """Load libqvq.so (built in-tree by __graft_entry__.build() / make -C quant_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QVQError(-1, "libqvq.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        P, u32, u64, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        sig = {
            "qvq_create": ([i, ctypes.POINTER(P)], i),
            "qvq_destroy": ([P], None),
            "qvq_last_error": ([P], ctypes.c_char_p),
            "qvq_version": ([], ctypes.c_char_p),
            "qvq_set_images": ([P, P, u32, u32, u32, u32, u32, i], i),
            "qvq_set_images_device": ([P, P, u32, u32, u32, u32, u32, i], i),
            "qvq_set_synthetic": ([P, u32, u64, u32, u32, u32, i], i),
            "qvq_set_vectors": ([P, P, u64, u32], i),
            "qvq_set_vectors_exact": ([P, P, u64, u32], i),
            "qvq_num_vectors": ([P], u64),
            "qvq_dim": ([P], u32),
            "qvq_lbg": ([P, u32, ctypes.c_double, P, P, P], i),
            "qvq_assign_device": ([P], P),
            "qvq_assign": ([P, P, u32, P], i),
            "qvq_update": ([P, P, u32, P, P], i),
            "qvq_update_kahan": ([P, P, u32, P], i),
            "qvq_update_kahan_split": ([P, P, u32, P, u32, P], i),
            "qvq_host_pool_stress": ([u32, u32, P], i),
            "qvq_comm_unique_id": ([P], i),
            "qvq_comm_init": ([P, i, i, P], i),
            "qvq_set_timing": ([P, i], i),
            "qvq_get_timings": ([P, ctypes.POINTER(_Timings)], i),
            "qvq_host_kdtree_nn": ([P, u32, u32, P, u64, P], i),
            "qvq_host_kdtree_image": ([P, u32, u32, P, u64, P], i),
            "qvq_kdtree_device_check": ([P, P, u32, u32, P, P], i),
            "qvq_host_finalize": ([P, P, P, u32, u32, i, P], i),
            "qvq_host_row_terms": ([P, u32, i, P, P], i),
            "qvq_decode": ([P, P, u32, P, u64, u32, u32, u32, u32, P], i),
            "qvq_decode_mse": ([P, P, u32, P, u64, u32, u32, u32, u32, P, P, P], i),
            "qvq_decode_device": ([P, P, u32, P, u64, u32, u32, u32, u32, P, P], i),
            "qvq_set_timeout": ([P, ctypes.c_double], i),
            "qvq_host_wait_probe": ([i, ctypes.c_double, P], i),
            "qvq_comm_init_host": ([P, i, i, ALLREDUCE_FN, P], i),
            "qvq_comm_info": ([P, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)], i),
            "qvq_refine": ([P, u32, P, u32, ctypes.c_double, u32, P, P, P, P, P, P], i),
            "qvq_host_plan": ([u32, u32, u64, ctypes.POINTER(_Plan)], i),
            "qvq_host_exact_plan": ([u32, u32, ctypes.POINTER(_ExactPlan)], i),
            "qvq_host_exact_grids": ([ctypes.POINTER(_ExactGrids)], i),
            "qvq_host_decode_plan": ([u32, u32, u32, u32, u32, u32, ctypes.POINTER(_DecodePlan)], i),
            "qvq_set_vectors_device": ([P, P, u64, u32, u32, P], i),
            "qvq_get_training_info": ([P, ctypes.POINTER(_TrainingInfo)], i),
            "qvq_get_ingest_ms": ([P, P], i),
            "qvq_host_colorspace_values": ([i, P], i),
            "qvq_host_classify": ([P, u64, u32, ctypes.POINTER(ctypes.c_int32), P], i),
            "qvq_host_ingest_grid": ([ctypes.POINTER(_IngestGrid)], i),
            "qvq_get_vectors": ([P, u64, u64, P], i),
            "qvq_host_cie1931": ([P, u64, P], i),
            "qvq_host_tile64_grid": ([ctypes.POINTER(_IngestGrid)], i),   # qvq_tile64_grid: the same two fields
            "qvq_get_refine_reseeds": ([P, P, u32, ctypes.POINTER(u32)], i),
            "qvq_host_row_error": ([P, P, u32, i, ctypes.POINTER(u32)], i),
            "qvq_host_reseed_far_key": ([u32, u32, ctypes.POINTER(u64)], i),
            "qvq_host_reseed_select": ([P, P, P, u32, P, P, ctypes.POINTER(u32)], i),
            "qvq_host_reseed_grid": ([ctypes.POINTER(_IngestGrid)], i),   # qvq_reseed_grid: the same two fields
            "qvq_median_cut": ([P, u32, P, P, P, P], i),
            "qvq_host_median_cut_plan": ([u32, u32, u64, ctypes.POINTER(_MedianCutPlan)], i),
            "qvq_host_median_cut_axis": ([P, P, u32, ctypes.POINTER(u32)], i),
            "qvq_host_median_cut_select": ([P, u32, u32, u64, ctypes.POINTER(u32)], i),
            "qvq_lbg_lloyd": ([P, u32, u32, ctypes.c_double, u32, P, P, P, P], i),
            "qvq_kmeanspp": ([P, u32, u64, P, P, P, P], i),
            "qvq_host_kmpp_draw": ([u64, u64, u64, ctypes.POINTER(u64)], i),
            "qvq_host_kmpp_weight": ([P, P, u32, ctypes.POINTER(u32)], i),
            "qvq_host_kmeanspp_plan": ([u64, ctypes.POINTER(_KMeansPPPlan)], i),
            "qvq_kmeanspp_greedy": ([P, u32, u64, u32, P, P, P, P, P, P, ctypes.POINTER(_KMeansPPGreedyInfo)], i),
            "qvq_host_kmpp_trials": ([u32, u32, ctypes.POINTER(u32)], i),
            "qvq_kmeans_par": ([P, u32, u64, ctypes.POINTER(_KMeansParOpts), P, P, P, P, ctypes.POINTER(_KMeansParInfo)], i),
            "qvq_host_kmeans_par_join": ([u64, u32, u64, u64, u32, u32, ctypes.POINTER(ctypes.c_int)], i),
            "qvq_host_kmeans_par_plan": ([u64, u32, u32, ctypes.POINTER(_KMeansParOpts), ctypes.POINTER(_KMeansParPlan)], i),
            "qvq_get_kahan_stats": ([P, ctypes.POINTER(_KahanStats)], i),
            "qvq_host_kahan_sort_plan": ([u32, ctypes.POINTER(_KahanSortPlan)], i),
            "qvq_host_mean_grid": ([u64, u32, ctypes.POINTER(_MeanGrid)], i),
        }
        for name, (args, res) in sig.items():
            if os.environ.get("QVQ_LIB") and not hasattr(L, name):
                continue   # an older A/B build (tools/) without this entry point
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(st, ctx=None):
    if st != 0:
        msg = lib().qvq_last_error(ctx)
        raise QVQError(st, msg.decode() if msg else "")


def _torch_runtime_first():
    """PyTorch-ROCm wheels bundle their own HIP/HSA runtime next to the /opt/rocm one libqvq.so
    links.  When libqvq.so opens the device first, the bundled runtime's later device discovery
    fails ("No HIP GPUs are available"); the other order works.  So if torch is already loaded,
    let it open the device before the engine does."""
    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:   # no device for torch: the engine's own error says why
            pass


class Engine:
    """One qvq context: one GPU, one HIP stream, one resident training set."""

    def __init__(self, device=0):
        _torch_runtime_first()
        h = ctypes.c_void_p()
        L = lib()
        _check(L.qvq_create(device, ctypes.byref(h)))
        self._h = h
        self._device = device
        self._L = L   # held by the engine: at interpreter shutdown the module globals may be gone

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._L.qvq_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001  (interpreter shutdown: nothing left to report to)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- training sets -------------------------------------------------------------------
    def set_images(self, rgb, n_images, xSize, ySize, bw, bh, colorspace=SCALED):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.size == n_images * xSize * ySize * 3
        _check(lib().qvq_set_images(self._h, _p(rgb), n_images, xSize, ySize, bw, bh, colorspace), self._h)

    def set_images_device(self, ptr, n_images, xSize, ySize, bw, bh, colorspace=SCALED):
        _check(lib().qvq_set_images_device(self._h, ctypes.c_void_p(ptr), n_images, xSize, ySize, bw, bh,
                                           colorspace), self._h)

    def set_synthetic(self, S, seed0=0x5EED, n_images=1, bw=2, bh=2, colorspace=SCALED):
        _check(lib().qvq_set_synthetic(self._h, S, seed0, n_images, bw, bh, colorspace), self._h)

    def set_vectors(self, X, exact=False):
        """fp64 training set N x dim.  Byte-image values (NORMAL/SCALED) take the fast path; any
        other data -- or exact=True -- the exact mode (the reference's Kahan arithmetic, qvq.h).
        X: anything numpy takes, or a torch tensor.  A CUDA tensor stays on the device
        (set_vectors_device with its data_ptr() and torch's current stream): it must be float64,
        2-D, contiguous and on the engine's GPU (QVQError QVQ_EINVAL otherwise, before anything
        reaches the library).  A CPU tensor goes through numpy."""
        if getattr(X, "is_cuda", False):
            import torch
            if (X.dtype != torch.float64 or X.dim() != 2 or not X.is_contiguous()
                    or X.device.index != self._device):
                raise QVQError(1, "a device tensor must be float64, 2-D, contiguous and on the engine's GPU")
            with torch.cuda.device(X.device):
                stream = torch.cuda.current_stream().cuda_stream
            return self.set_vectors_device(X.data_ptr(), X.shape[0], X.shape[1], exact=exact, stream=stream)
        if hasattr(X, "is_cuda"):   # a CPU tensor
            X = X.detach().numpy()
        X = np.ascontiguousarray(X, np.float64)
        fn = lib().qvq_set_vectors_exact if exact else lib().qvq_set_vectors
        _check(fn(self._h, _p(X), X.shape[0], X.shape[1]), self._h)

    def set_vectors_device(self, ptr, n, dim, exact=False, stream=None):
        """fp64 rows n x dim already in device memory (qvq_set_vectors_device): ptr their address,
        stream the hipStream_t handle whose queued work produces them (None or 0 = the legacy null
        stream).  The rows may be overwritten or freed once this returns."""
        _check(lib().qvq_set_vectors_device(self._h, ctypes.c_void_p(ptr), n, dim, VECTORS_EXACT if exact else 0,
                                            ctypes.c_void_p(stream or 0)), self._h)

    def training_info(self):
        """What is resident (qvq_get_training_info): {"mode": MODE_NONE / MODE_BYTE / MODE_EXACT,
        "colorspace": NORMAL / SCALED on the byte path, CIE1931 for an exact set from a CIE1931
        raster, -1 for one from set_vectors or none, "n", "dim"}."""
        t = _TrainingInfo()
        _check(lib().qvq_get_training_info(self._h, ctypes.byref(t)), self._h)
        return {"mode": int(t.mode), "colorspace": int(t.colorspace), "n": int(t.n), "dim": int(t.dim)}

    def get_vectors(self, row0=0, nrows=None):
        """The resident rows row0 .. row0 + nrows - 1 (default: to the end) as float64 [nrows, dim]
        (qvq_get_vectors): exact mode's rows themselves, the byte path's values without padding."""
        row0 = int(row0)
        nrows = self.n - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0:
            raise QVQError(1, "rows outside the training set")
        out = np.empty((nrows, self.dim), np.float64)
        _check(lib().qvq_get_vectors(self._h, row0, nrows, _p(out)), self._h)
        return out

    def ingest_ms(self):
        """(classify ms, pack ms) of the last set_vectors* call's device passes, under set_timing(-3)."""
        ms = np.zeros(2, np.float64)
        _check(lib().qvq_get_ingest_ms(self._h, _p(ms)), self._h)
        return float(ms[0]), float(ms[1])

    @property
    def n(self):
        return int(lib().qvq_num_vectors(self._h))

    @property
    def dim(self):
        return int(lib().qvq_dim(self._h))

    # -- hot path ------------------------------------------------------------------------
    def lbg(self, bits, eps=1e-6, want_assign=True, out=None):
        """Split-LBG to 2**bits code vectors: (codebook, indices or None, distortion).
        out: optional (C, d) float64 arrays of shapes (2**bits, dim) and (1,) to fill instead of
        allocating (repeated calls, e.g. bench.py)."""
        K = 1 << bits
        if out is None:
            C, d = np.empty((K, self.dim), np.float64), np.zeros(1, np.float64)
        else:
            C, d = out
            assert C.shape == (K, self.dim) and C.dtype == np.float64 and C.flags.c_contiguous
            assert d.shape == (1,) and d.dtype == np.float64
        A = np.empty(self.n, np.uint32) if want_assign else None
        _check(lib().qvq_lbg(self._h, bits, eps, _p(C), _p(A) if want_assign else None, _p(d)), self._h)
        self._last_k = K
        return C, A, float(d[0])

    def refine(self, K=None, C=None, max_iters=100, eps=1e-6, fresh=False, want_assign=True, reseed=False):
        """Lloyd refinement at fixed K on the device (qvq_refine): (C, A, distortion, info).
        C=None continues from this engine's last lbg() or refine() (K defaults to that call's K);
        a K x dim array C is a warm start.  fresh=True returns the indices of the final codebook
        (one more assignment) and their distortion.  info: iters, stop (STOP_FIXED / STOP_EPS /
        STOP_MAXIT), changed (rows that moved, per iteration), distortion (per iteration), reseeded
        (seeds placed, per iteration: all 0 without reseed).  reseed=True: after each centroid step
        the empty cells take rows of the worst cells (QVQ_REFINE_RESEED; one rank's byte path).
        want_assign=False leaves the indices on the device (A is None).
        With a communicator joined (comm_init / comm_init_host) every rank calls it with the same
        arguments on its own rows: C, distortion and info are those of one rank over all the rows,
        bit for bit and the same on every rank (changed counts every rank's rows), A is this rank's
        rows.  A rank whose call is invalid raises its own status, its peers QVQ_EINVAL."""
        if C is not None:
            C = np.ascontiguousarray(C, np.float64)
            if C.ndim != 2 or C.shape[1] != self.dim or (K is not None and K != C.shape[0]):
                raise QVQError(1, "starting codebook must be K x dim")
            K = C.shape[0]
        elif K is None:
            K = getattr(self, "_last_k", 0)
        max_iters = int(max_iters)
        out = np.empty((K, self.dim), np.float64)
        A = np.empty(self.n, np.uint32) if want_assign else None
        d = np.zeros(1, np.float64)
        chg = np.zeros(max(max_iters, 1), np.uint64)
        trace = np.zeros(max(max_iters, 1), np.float64)
        seeds = np.zeros(max(max_iters, 1), np.uint64)
        inf = np.zeros(2, np.uint32)
        _check(lib().qvq_refine(self._h, K, _p(C) if C is not None else None, max_iters, float(eps),
                                (REFINE_FRESH if fresh else 0) | (REFINE_RESEED if reseed else 0), _p(out),
                                _p(A) if want_assign else None, _p(d), _p(chg), _p(trace), _p(inf)),
               self._h)
        self._last_k = K
        it = int(inf[0])
        if hasattr(lib(), "qvq_get_refine_reseeds"):   # (an older A/B build, QVQ_LIB, has none: it never seeds)
            _check(lib().qvq_get_refine_reseeds(self._h, _p(seeds), seeds.size, None), self._h)
        return out, A, float(d[0]), {"iters": it, "stop": int(inf[1]), "changed": [int(x) for x in chg[:it]],
                                     "distortion": [float(x) for x in trace[:it]],
                                     "reseeded": [int(x) for x in seeds[:it]]}

    def lbg_lloyd(self, bits, iters, eps=1e-6, reseed=False, want_assign=True):
        """Split-LBG with up to `iters` Lloyd iterations at every level, stopped by eps
        (qvq_lbg_lloyd, the rule in qvq.h): (C, A or None, distortion, levels), levels[l] a dict of
        level l + 1's iters, stop (STOP_*), changed (rows changed in its last iteration), empty
        (cells without a row), seeds (placed at the level: 0 without reseed) and distortion.
        reseed=True: every level's iterations reseed their empty cells (QVQ_LLOYD_RESEED).  One
        rank's byte path.  refine(C=None) continues from the result."""
        bits = int(bits)
        K = 1 << bits
        C, d = np.empty((K, self.dim), np.float64), np.zeros(1, np.float64)
        A = np.empty(self.n, np.uint32) if want_assign else None
        lv = (_LloydLevel * max(bits, 1))()
        _check(lib().qvq_lbg_lloyd(self._h, bits, int(iters), float(eps), LLOYD_RESEED if reseed else 0, _p(C),
                                   _p(A) if want_assign else None, _p(d), ctypes.cast(lv, ctypes.c_void_p)), self._h)
        self._last_k = K
        return C, A, float(d[0]), [{"iters": int(v.iters), "stop": int(v.stop), "changed": int(v.changed),
                                    "empty": int(v.empty), "seeds": int(v.seeds), "distortion": float(v.distortion)}
                                   for v in lv[:bits]]

    def median_cut(self, bits, want_assign=True):
        """Median cut to 2**bits boxes on the device (qvq_median_cut, the rule in qvq.h): (codebook,
        labels or None, distortion, cuts), cuts[l] the boxes cut at level l + 1.  One rank's byte
        path.  The codebook is a warm start for refine(C=...); refine(C=None) cannot continue from it."""
        K = 1 << bits
        C, d = np.empty((K, self.dim), np.float64), np.zeros(1, np.float64)
        A = np.empty(self.n, np.uint32) if want_assign else None
        cuts = np.zeros(max(bits, 1), np.uint32)
        _check(lib().qvq_median_cut(self._h, bits, _p(C), _p(A) if want_assign else None, _p(d), _p(cuts)), self._h)
        return C, A, float(d[0]), [int(x) for x in cuts[:bits]]

    def kmeanspp(self, K, seed=0):
        """k-means++ seeding on the device (qvq_kmeanspp, the rule in qvq.h): (codebook, rows,
        potential, placed).  codebook[j] holds the values of training row rows[j] for j < placed
        and zeros after; rows[j] is 0xFFFFFFFF and potential[j] 0 from placed on.  potential[j] / n
        is the mean squared error of seeds 0 .. j in squared ordinal units.  Any K in 1 .. 2**20;
        one rank's byte path.  The codebook is a start for refine(C=...); nothing resident changes."""
        K = int(K)
        if K <= 0:
            raise QVQError(1, "K must be in 1 .. 2^20")
        C = np.empty((K, self.dim), np.float64)
        rows, pot = np.empty(K, np.uint32), np.empty(K, np.uint64)
        placed = ctypes.c_uint32()
        _check(lib().qvq_kmeanspp(self._h, K, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(C), _p(rows), _p(pot),
                                  ctypes.cast(ctypes.byref(placed), ctypes.c_void_p)), self._h)
        return C, rows, pot, int(placed.value)

    def kmeanspp_greedy(self, K, seed=0, trials=0):
        """Greedy k-means++ seeding on the device (qvq_kmeanspp_greedy, the rule in qvq.h): every round
        draws `trials` candidate rows (0: the default 2 + 7 floor(log2 K) / 10, at most 16) and keeps
        the one that lowers the potential most.  Returns (codebook, rows, potential, info): codebook,
        rows and potential as kmeanspp's; info is a dict of placed, trials (the count used), trial
        [K] (the winning trial of every round), trial_rows and trial_potential [K, 16] (every
        candidate's row and potential; 0xFFFFFFFF and 0 where a round had no such trial).  trials = 1
        is kmeanspp.  Nothing resident changes."""
        K = int(K)
        if K <= 0:
            raise QVQError(1, "K must be in 1 .. 2^20")
        if not 0 <= int(trials) <= 16:
            raise QVQError(1, "trials must be in 0 .. 16")
        C = np.empty((K, self.dim), np.float64)
        rows, pot, trial = np.empty(K, np.uint32), np.empty(K, np.uint64), np.empty(K, np.uint32)
        trows, tpot = np.empty((K, 16), np.uint32), np.empty((K, 16), np.uint64)
        info = _KMeansPPGreedyInfo()
        _check(lib().qvq_kmeanspp_greedy(self._h, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(trials), _p(C), _p(rows),
                                         _p(pot), _p(trial), _p(trows), _p(tpot), ctypes.byref(info)), self._h)
        return C, rows, pot, {"placed": int(info.placed), "trials": int(info.trials), "trial": trial,
                              "trial_rows": trows, "trial_potential": tpot}

    def kmeans_par(self, K, seed=0, rounds=0, ell=0, round_cap=0):
        """k-means|| seeding on the device (qvq_kmeans_par, the rule in qvq.h): (codebook, rows,
        cand_rows, cand_weights, info).  A 0 option is its default (rounds 5, ell K, round_cap
        2 ell + 64).  codebook[j] holds the values of training row rows[j] for j < info["placed"] and
        zeros after; rows[j] is 0xFFFFFFFF from placed on.  cand_rows and cand_weights have
        host_kmeans_par_plan's max_candidates entries, 0xFFFFFFFF and 0 from info["candidates"] on.
        info: placed, candidates, rounds_run, truncated, round_candidates (16) and potential (17) as
        lists.  K in 1 .. 2**16; one rank's byte path.  The codebook is a start for refine(C=...);
        nothing resident changes."""
        K = int(K)
        opts = _KMeansParOpts(int(rounds), int(ell), int(round_cap))
        try:
            n_cand = host_kmeans_par_plan(max(self.n, 1), self.dim or 1, K, rounds, ell, round_cap)["max_candidates"]
        except QVQError:
            n_cand = 1   # outside the limits: the call below reports it, in the contract's order
        C = np.empty((max(K, 0), self.dim), np.float64)
        rows, crows, cwt = np.empty(K, np.uint32), np.empty(n_cand, np.uint32), np.empty(n_cand, np.uint64)
        info = _KMeansParInfo()
        _check(lib().qvq_kmeans_par(self._h, K, int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(opts), _p(C), _p(rows),
                                    _p(crows), _p(cwt), ctypes.byref(info)), self._h)
        return C, rows, crows, cwt, _kmeans_par_info(info)

    def refine_reseeds(self):
        """The seeds the last refine() placed in each iteration (qvq_get_refine_reseeds)."""
        n = ctypes.c_uint32()
        _check(lib().qvq_get_refine_reseeds(self._h, None, 0, ctypes.byref(n)), self._h)
        out = np.zeros(max(n.value, 1), np.uint64)
        _check(lib().qvq_get_refine_reseeds(self._h, _p(out), n.value, ctypes.byref(n)), self._h)
        return [int(x) for x in out[:n.value]]

    def assign(self, C):
        C = np.ascontiguousarray(C, np.float64)
        A = np.empty(self.n, np.uint32)
        _check(lib().qvq_assign(self._h, _p(C), C.shape[0], _p(A)), self._h)
        return A

    def update(self, A, K):
        A = np.ascontiguousarray(A, np.uint32)
        C = np.empty((K, self.dim), np.float64)
        cnt = np.empty(K, np.uint64)
        _check(lib().qvq_update(self._h, _p(A), K, _p(C), _p(cnt)), self._h)
        return C, cnt

    def update_kahan(self, A, K):
        """The reference's centroid bits (Kahan sums in row order, src/Quantizer.cpp:59-87)."""
        A = np.ascontiguousarray(A, np.uint32)
        C = np.empty((K, self.dim), np.float64)
        _check(lib().qvq_update_kahan(self._h, _p(A), K, _p(C)), self._h)
        return C

    def update_kahan_split(self, A, K, splits):
        """update_kahan with the rows cut into virtual ranks at splits (0 .. n): the several-rank
        chained evaluation run rank after rank on this device (test entry)."""
        A = np.ascontiguousarray(A, np.uint32)
        sp = np.ascontiguousarray(splits, np.uint64)
        C = np.empty((K, self.dim), np.float64)
        _check(lib().qvq_update_kahan_split(self._h, _p(A), K, _p(sp), sp.size - 1, _p(C)), self._h)
        return C

    def kahan_stats(self):
        """What the last update_kahan / update_kahan_split ran (qvq_get_kahan_stats, test entry): a
        dict of the qvq_kahan_stats fields; route is one of KAHAN_ROUTE_*."""
        st = _KahanStats()
        _check(lib().qvq_get_kahan_stats(self._h, ctypes.byref(st)), self._h)
        return {f: int(getattr(st, f)) for f, _ in _KahanStats._fields_}

    def assign_device_ptr(self):
        return lib().qvq_assign_device(self._h)

    def kdtree_device_check(self, C):
        """The reference kd-tree of C (K x D) built on the device against the host's, node for node:
        (result, [launch ms, phase-1 ms, phase-2 ms, images ms], first difference); result 0 equal,
        1 different, 2 the build gave up."""
        C = np.ascontiguousarray(C, np.float64)
        ms = np.zeros(4, np.float64)
        res = np.zeros(1, np.uint32)
        _check(lib().qvq_kdtree_device_check(self._h, _p(C), C.shape[0], C.shape[1], _p(ms), _p(res)), self._h)
        why = lib().qvq_last_error(self._h).decode() if res[0] == 1 else ""
        return int(res[0]), [round(float(x), 4) for x in ms], why

    def set_timing(self, level=-1):
        """HIP events around the search of every level (-1), none (-2) or level+1 only."""
        _check(lib().qvq_set_timing(self._h, int(level)), self._h)

    def level_timing(self, level):
        """(search ms, update ms, flagged rows over all levels) of the last lbg, without
        building the full timings() dict (bench.py reads this once per step)."""
        t = getattr(self, "_tm", None)
        if t is None:
            t = self._tm = _Timings()
        _check(lib().qvq_get_timings(self._h, ctypes.byref(t)), self._h)
        return t.assign_ms[level], t.update_ms[level], sum(t.flagged[:max(t.levels, 1)])

    def timings(self):
        t = _Timings()
        _check(lib().qvq_get_timings(self._h, ctypes.byref(t)), self._h)
        L = t.levels
        return {"levels": L, "total_ms": t.total_ms,
                "assign_ms": list(t.assign_ms[:max(L, 1)]), "update_ms": list(t.update_ms[:max(L, 1)]),
                "other_ms": list(t.other_ms[:max(L, 1)]),
                "flagged": list(t.flagged[:max(L, 1)]), "host_ties": list(t.host_ties[:max(L, 1)]),
                "wait_ms": list(t.wait_ms[:max(L, 1)]), "tree_ms": list(t.tree_ms[:max(L, 1)]),
                "kahan_redo": t.kahan_redo, "tie_overflow": t.tie_overflow, "kahan_relays": t.kahan_relays,
                "mean_ms": t.mean_ms}

    # -- multi-GPU -----------------------------------------------------------------------
    def decode(self, cb_bytes, A, xSize, ySize, bw, bh):
        """CompressedImage::decompress (src/Compressor.cpp:156-165) on the device: codebook bytes
        (K x bw*bh*3 u8) and block indices -> xSize*ySize*3 raster (u8)."""
        cb = np.ascontiguousarray(cb_bytes, dtype=np.uint8).reshape(-1, bw * bh * 3)
        A = np.ascontiguousarray(A, dtype=np.uint32).ravel()
        out = np.empty(xSize * ySize * 3, dtype=np.uint8)
        _check(lib().qvq_decode(self._h, _p(cb), cb.shape[0], _p(A), A.size, xSize, ySize, bw, bh, _p(out)), self._h)
        return out

    def decode_mse(self, cb_bytes, A, xSize, ySize, bw, bh, orig, want_image=True):
        """Decode plus the raport's distortion (src/Compressor.cpp:133-146): mean squared
        difference of the signed bytes of orig and the decoded raster, in the same device pass.
        Returns (raster or None, mse)."""
        cb = np.ascontiguousarray(cb_bytes, dtype=np.uint8).reshape(-1, bw * bh * 3)
        A = np.ascontiguousarray(A, dtype=np.uint32).ravel()
        orig = np.ascontiguousarray(orig, dtype=np.uint8).ravel()
        assert orig.size == xSize * ySize * 3
        out = np.empty(xSize * ySize * 3, dtype=np.uint8) if want_image else None
        mse = ctypes.c_double()
        _check(lib().qvq_decode_mse(self._h, _p(cb), cb.shape[0], _p(A), A.size, xSize, ySize, bw, bh,
                                    _p(out) if want_image else None, _p(orig), ctypes.byref(mse)), self._h)
        return out, mse.value

    def set_timeout(self, seconds):
        """Bound of every host wait on the engine's stream (QVQ_ECOMM / QVQ_EDEVICE past it)."""
        _check(lib().qvq_set_timeout(self._h, float(seconds)), self._h)

    def decode_device(self, cb_ptr, K, a_ptr, nblocks, xSize, ySize, bw, bh, rgb_ptr, stream=None):
        """Device-pointer decode on `stream` (a hipStream_t handle; None or 0 = the legacy null
        stream, ordered after the caller's work on blocking streams)."""
        _check(lib().qvq_decode_device(self._h, cb_ptr, K, a_ptr, nblocks, xSize, ySize, bw, bh, rgb_ptr, stream),
               self._h)

    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check(lib().qvq_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().qvq_comm_init(self._h, nranks, rank, buf), self._h)

    def comm_init_host(self, nranks, rank, allreduce):
        """Test-only communicator (qvq_comm_init_host): allreduce(arr) must replace the numpy
        array arr (uint64 or float64) in place by its sum over the ranks, e.g. through
        torch.distributed's gloo backend.  Lets several processes share one GPU."""
        def cb(ptr, count, dtype, user):
            try:
                ct = ctypes.c_uint64 if dtype == 0 else ctypes.c_double
                arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), shape=(count,))
                allreduce(arr)
                return 0
            except Exception:   # noqa: BLE001  (no exception may cross the C ABI)
                import traceback
                traceback.print_exc()
                return 1
        self._ar_cb = ALLREDUCE_FN(cb)   # kept alive with the engine
        _check(lib().qvq_comm_init_host(self._h, nranks, rank, self._ar_cb, None), self._h)

    def comm_info(self):
        """(nranks, rank, kind) of the joined communicator; kind COMM_NONE/COMM_RCCL/COMM_HOST."""
        n, r, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().qvq_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(k)), self._h)
        return n.value, r.value, k.value


# -- host-only helpers (no GPU) ------------------------------------------------------------
def host_kdtree_nn(C, Q):
    C = np.ascontiguousarray(C, np.float64)
    Q = np.ascontiguousarray(Q, np.float64)
    out = np.empty(Q.shape[0], np.uint32)
    _check(lib().qvq_host_kdtree_nn(_p(C), C.shape[0], C.shape[1], _p(Q), Q.shape[0], _p(out)))
    return out


def host_plan(dim, K, n):
    """The kernels the engine dispatches to for n rows of dim components and K code vectors
    (qvq_host_plan, under the current QVQ_SEARCH / QVQ_KDTREE): a dict of the qvq_plan fields."""
    p = _Plan()
    _check(lib().qvq_host_plan(int(dim), int(K), int(n), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _Plan._fields_}


def host_exact_plan(dim, K):
    """The exact mode's dispatch for dim components and K code vectors (qvq_host_exact_plan): a dict
    of the qvq_exact_plan fields."""
    p = _ExactPlan()
    _check(lib().qvq_host_exact_plan(int(dim), int(K), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _ExactPlan._fields_}


def host_decode_plan(K, xSize, ySize, bw, bh, align_flags=0):
    """The kernel a decode of this shape dispatches to (qvq_host_decode_plan): a dict of the
    qvq_decode_plan fields.  align_flags: the DECODE_*_UNALIGNED / DECODE_CODEBOOK_ODD bits of what
    qvq_decode_device's pointers lack; 0 for the host entry points."""
    p = _DecodePlan()
    _check(lib().qvq_host_decode_plan(int(K), int(xSize), int(ySize), int(bw), int(bh), int(align_flags),
                                      ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _DecodePlan._fields_}


def host_exact_grids():
    """The exact kernels' grid caps (qvq_host_exact_grids): a dict of the qvq_exact_grids fields."""
    g = _ExactGrids()
    _check(lib().qvq_host_exact_grids(ctypes.byref(g)))
    return {f: int(getattr(g, f)) for f, _ in _ExactGrids._fields_}


def host_ingest_grid():
    """The fp64 front door's launch shape (qvq_host_ingest_grid): {"block", "blocks"}; one lane per
    4-byte code word."""
    g = _IngestGrid()
    _check(lib().qvq_host_ingest_grid(ctypes.byref(g)))
    return {f: int(getattr(g, f)) for f, _ in _IngestGrid._fields_}


def host_kahan_sort_plan(K):
    """The key windows of the Kahan centroids' sort by cell over K keys (qvq_host_kahan_sort_plan): a
    dict of the qvq_kahan_sort_plan fields."""
    p = _KahanSortPlan()
    _check(lib().qvq_host_kahan_sort_plan(int(K), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _KahanSortPlan._fields_}


def host_tile64_grid():
    """The tile-to-fp64 kernel's launch shape (qvq_host_tile64_grid): {"block", "blocks"}; one lane per
    (row, pixel in block) slot."""
    g = _IngestGrid()
    _check(lib().qvq_host_tile64_grid(ctypes.byref(g)))
    return {f: int(getattr(g, f)) for f, _ in _IngestGrid._fields_}


def host_cie1931(rgb):
    """The CIE1931 map of set_images on the host (qvq_host_cie1931): rgb [..., 3] uint8 (read as signed
    chars) -> float64 [npix, 3]."""
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    out = np.empty((rgb.shape[0], 3), np.float64)
    _check(lib().qvq_host_cie1931(_p(rgb), rgb.shape[0], _p(out)))
    return out


def host_reseed_grid():
    """The reseed rows pass's launch shape (qvq_host_reseed_grid): {"block", "blocks"}; one lane per row."""
    g = _IngestGrid()
    _check(lib().qvq_host_reseed_grid(ctypes.byref(g)))
    return {f: int(getattr(g, f)) for f, _ in _IngestGrid._fields_}


def host_median_cut_plan(dim, boxes, n):
    """One median-cut level of `boxes` boxes over n rows of dim components (qvq_host_median_cut_plan):
    a dict of the qvq_median_cut_plan fields."""
    p = _MedianCutPlan()
    _check(lib().qvq_host_median_cut_plan(int(dim), int(boxes), int(n), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _MedianCutPlan._fields_}


def host_median_cut_axis(lo, hi):
    """The cut axis of a box from its per-component minima and maxima (qvq_host_median_cut_axis)."""
    lo = np.ascontiguousarray(lo, np.uint32).ravel()
    hi = np.ascontiguousarray(hi, np.uint32).ravel()
    assert lo.size == hi.size
    axis = ctypes.c_uint32()
    _check(lib().qvq_host_median_cut_axis(_p(lo), _p(hi), lo.size, ctypes.byref(axis)))
    return axis.value


def host_median_cut_select(hist, lo, hi, n=None):
    """The cut t of a box from its 256-bin histogram on the axis (qvq_host_median_cut_select); n
    defaults to the histogram's total."""
    hist = np.ascontiguousarray(hist, np.uint32).ravel()
    assert hist.size == 256
    t = ctypes.c_uint32()
    _check(lib().qvq_host_median_cut_select(_p(hist), int(lo), int(hi), int(hist.sum()) if n is None else int(n),
                                            ctypes.byref(t)))
    return t.value


def host_kmpp_draw(seed, j, T):
    """draw(seed, j, T) of qvq_kmeanspp's rule (qvq_host_kmpp_draw): an int in [0, T)."""
    t = ctypes.c_uint64()
    _check(lib().qvq_host_kmpp_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(j), int(T), ctypes.byref(t)))
    return int(t.value)


def host_kmpp_weight(codes_a, codes_b):
    """w(a, b) of qvq_kmeanspp's rule from two rows' code bytes, pad bytes included (qvq_host_kmpp_weight)."""
    a = np.ascontiguousarray(codes_a, np.uint8).ravel()
    b = np.ascontiguousarray(codes_b, np.uint8).ravel()
    assert a.size == b.size
    w = ctypes.c_uint32()
    _check(lib().qvq_host_kmpp_weight(_p(a), _p(b), a.size, ctypes.byref(w)))
    return int(w.value)


def host_kmpp_trials(K, trials=0):
    """The trial count qvq_kmeanspp_greedy uses for K seeds (qvq_host_kmpp_trials): `trials`, or for 0
    the default 2 + 7 floor(log2 K) / 10.  QVQError where the call gives QVQ_EINVAL."""
    K, trials = int(K), int(trials)
    if not (0 <= K < 1 << 32 and 0 <= trials < 1 << 32):
        raise QVQError(1, "K must be in 1 .. 2^20 and trials in 0 .. 16")
    L = ctypes.c_uint32()
    _check(lib().qvq_host_kmpp_trials(K, trials, ctypes.byref(L)))
    return int(L.value)


def _kmeans_par_info(info):
    return {"placed": int(info.placed), "candidates": int(info.candidates), "rounds_run": int(info.rounds_run),
            "truncated": int(info.truncated), "round_candidates": [int(v) for v in info.round_candidates],
            "potential": [int(v) for v in info.potential]}


def host_kmeans_par_join(seed, r, row, phi, ell, m):
    """The sampling test of qvq_kmeans_par's rule (qvq_host_kmeans_par_join): does `row` with weight m
    join round r under potential phi."""
    j = ctypes.c_int()
    _check(lib().qvq_host_kmeans_par_join(int(seed) & 0xFFFFFFFFFFFFFFFF, int(r), int(row), int(phi), int(ell), int(m),
                                          ctypes.byref(j)))
    return bool(j.value)


def host_kmeans_par_plan(n, dim, K, rounds=0, ell=0, round_cap=0):
    """qvq_kmeans_par's options with the defaults filled in and its launch shape over n rows of dim
    components (qvq_host_kmeans_par_plan): a dict of rounds, ell, round_cap, block, segments, seg_rows,
    segments_cap, chunk, max_candidates, reduce_block, gw_lds, codes_lds, lds_bytes.  Raises QVQError
    (status 1) outside the contract's limits."""
    p = _KMeansParPlan()
    opts = _KMeansParOpts(int(rounds), int(ell), int(round_cap))
    _check(lib().qvq_host_kmeans_par_plan(int(n), int(dim), int(K), ctypes.byref(opts), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _KMeansParPlan._fields_}


def host_kmeanspp_plan(n):
    """The launch shape of qvq_kmeanspp's update pass over n rows (qvq_host_kmeanspp_plan): a dict of
    block, segments, seg_rows, segments_cap."""
    p = _KMeansPPPlan()
    _check(lib().qvq_host_kmeanspp_plan(int(n), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _KMeansPPPlan._fields_}


def host_mean_grid(n, dim):
    """The launch shape of the K = 1 sums (the mean) over n rows of dim components
    (qvq_host_mean_grid): a dict of blocks, block, group_rows, chunk_groups, chunks_in_flight,
    groups_in_flight, chunk_loop."""
    p = _MeanGrid()
    _check(lib().qvq_host_mean_grid(int(n), int(dim), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in _MeanGrid._fields_}


def host_row_error(x, c, colorspace=SCALED):
    """The quantised per-row error of QVQ_REFINE_RESEED (qvq_host_row_error): values x against code vector c."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    c = np.ascontiguousarray(c, np.float64).ravel()
    assert x.size == c.size
    q = ctypes.c_uint32()
    _check(lib().qvq_host_row_error(_p(x), _p(c), x.size, int(colorspace), ctypes.byref(q)))
    return q.value


def host_reseed_far_key(q, row):
    """The far-row key (qvq_host_reseed_far_key): its maximum over a cell's rows names the far row."""
    key = ctypes.c_uint64()
    _check(lib().qvq_host_reseed_far_key(int(q), int(row), ctypes.byref(key)))
    return key.value


def host_reseed_select(E, n, far):
    """QVQ_REFINE_RESEED's selection (qvq_host_reseed_select) from the cells' summed errors E, row
    counts n and far-row keys far: (empties, rows), cell empties[j] takes row rows[j]."""
    E = np.ascontiguousarray(E, np.uint64)
    n = np.ascontiguousarray(n, np.uint64)
    far = np.ascontiguousarray(far, np.uint64)
    K = E.size
    assert n.size == K and far.size == K
    em, rows, m = np.zeros(K, np.uint32), np.zeros(K, np.uint32), ctypes.c_uint32()
    _check(lib().qvq_host_reseed_select(_p(E), _p(n), _p(far), K, _p(em), _p(rows), ctypes.byref(m)))
    return [int(x) for x in em[:m.value]], [int(x) for x in rows[:m.value]]


def colorspace_values(colorspace=SCALED):
    """The colour space's byte -> value table (qvq_host_colorspace_values): 256 float64, the values
    a byte-image training set must hold bit for bit."""
    out = np.empty(256, np.float64)
    _check(lib().qvq_host_colorspace_values(int(colorspace), _p(out)))
    return out


def host_classify(X, want_codes=True):
    """The value -> code rule of set_vectors on the host (qvq_host_classify): (colour space or -1,
    codes [n, Dp] uint8 or None)."""
    X = np.ascontiguousarray(X, np.float64)
    n, dim = X.shape
    cs = ctypes.c_int32(-2)
    codes = np.zeros((n, (dim + 3) & ~3), np.uint8) if want_codes else None
    _check(lib().qvq_host_classify(_p(X), n, dim, ctypes.byref(cs), _p(codes) if want_codes else None))
    return cs.value, (codes if want_codes and cs.value >= 0 else None)


# KdbNode (kdtree_dev.hpp) and the image layout of qvq_host_kdtree_image
KDB_NODE = np.dtype([("child1", "<i4"), ("child2", "<i4"), ("left", "<u4"), ("right", "<u4"), ("divfeat", "<i4"),
                     ("depth", "<u4"), ("divlow", "<f8"), ("divhigh", "<f8"), ("cutval", "<f8"),
                     ("split_val", "<f8"), ("spread_gap", "<f8"), ("cand", "<u8")])
KDB_HEADER_BYTES = 64


def host_kdtree_image(C):
    """The host build of C's kd-tree (RefKDTree) as arrays: (nodes [n] KDB_NODE breadth first,
    lo [n, D], hi [n, D] point boxes, vind [K], depth)."""
    C = np.ascontiguousarray(C, np.float64)
    K, D = C.shape
    need = ctypes.c_uint64()
    lib().qvq_host_kdtree_image(_p(C), K, D, None, 0, ctypes.byref(need))
    img = np.zeros(need.value, np.uint8)
    _check(lib().qvq_host_kdtree_image(_p(C), K, D, _p(img), img.size, ctypes.byref(need)))
    n_nodes, depth = (int(x) for x in img[:8].view("<u4"))
    off = KDB_HEADER_BYTES
    nodes = img[off:off + 2 * K * KDB_NODE.itemsize].view(KDB_NODE)[:n_nodes]
    off += 2 * K * KDB_NODE.itemsize
    boxes = img[off:off + 2 * K * 2 * D * 8].view("<f8").reshape(2 * K, 2, D)[:n_nodes]
    off += 2 * K * 2 * D * 8
    vind = img[off:off + 4 * K].view("<u4")
    return nodes, boxes[:, 0], boxes[:, 1], vind.copy(), depth


def host_wait_probe(scenario, timeout_s):
    """The engine's bounded-wait policy under scripted probes (qvq.h): (status, seconds)."""
    el = ctypes.c_double()
    st = lib().qvq_host_wait_probe(int(scenario), float(timeout_s), ctypes.byref(el))
    return st, el.value


def host_pool_stress(rounds, maxn):
    """The certificate's thread pool under jobs of changing width (qvq.h): slots run != once."""
    bad = ctypes.c_uint64()
    _check(lib().qvq_host_pool_stress(int(rounds), int(maxn), ctypes.byref(bad)))
    return bad.value


def host_finalize(hi, lo, cnt, colorspace=SCALED):
    hi = np.ascontiguousarray(hi, np.uint64)
    lo = np.ascontiguousarray(lo, np.uint64)
    cnt = np.ascontiguousarray(cnt, np.uint64)
    K, D = hi.shape
    C = np.empty((K, D), np.float64)
    _check(lib().qvq_host_finalize(_p(hi), _p(lo), _p(cnt), K, D, colorspace, _p(C)))
    return C


def host_row_terms(codes, colorspace=SCALED):
    """(hi, lo) exact-sum terms of each byte code, shape like codes (uint64)."""
    codes = np.ascontiguousarray(codes, np.uint8)
    flat = codes.reshape(-1)
    hi = np.empty(flat.size, np.uint64)
    lo = np.empty(flat.size, np.uint64)
    _check(lib().qvq_host_row_terms(_p(flat), flat.size, colorspace, _p(hi), _p(lo)))
    return hi.reshape(codes.shape), lo.reshape(codes.shape)


# -- the reference's plugin interface (include/Quantizer.hpp:8-20) ---------------------------
class Quantizers(enum.IntEnum):
    LBG = 0
    MEDIAN_CUT = 1
    LBG_MEDIAN_CUT = 2
    ABC = 3


class AbstractQuantizer:
    def quantize(self, trainingSet, n, eps):
        raise NotImplementedError


class LBGQuantizer(AbstractQuantizer):
    """LBGQuantizer (src/Quantizer.cpp:119-144) on the MI355X engine."""

    def __init__(self, device=0, refine_iters=0, fresh=False, reseed=False, lloyd_iters=0):
        """refine_iters > 0: up to that many Lloyd iterations at the final K after the split
        levels, stopped by eps (Engine.refine); fresh: the indices of the returned codebook;
        lloyd_iters > 0: up to that many Lloyd iterations after every split, stopped by eps
        (Engine.lbg_lloyd in place of Engine.lbg); reseed: the iterations reseed their empty cells
        (needs refine_iters > 0 or lloyd_iters > 0)."""
        if int(lloyd_iters) < 0:
            raise QVQError(1, "lloyd_iters must be >= 0")
        if reseed and int(refine_iters) <= 0 and int(lloyd_iters) <= 0:
            raise QVQError(1, "reseed needs refine_iters > 0 or lloyd_iters > 0")
        self._device = device
        self._engine = None
        self._refine_iters = int(refine_iters)
        self._fresh = bool(fresh)
        self._reseed = bool(reseed)
        self._lloyd_iters = int(lloyd_iters)

    def quantize(self, trainingSet, n, eps):
        if self._engine is None:
            self._engine = Engine(self._device)
        # a CUDA tensor goes straight through (no torch import here when handed numpy)
        dev = getattr(trainingSet, "is_cuda", False)
        self._engine.set_vectors(trainingSet if dev else np.asarray(trainingSet, np.float64))
        if self._lloyd_iters > 0:
            res = self._engine.lbg_lloyd(int(n), self._lloyd_iters, eps, reseed=self._reseed)[:3]
        else:
            res = self._engine.lbg(int(n), eps)
        if self._refine_iters > 0 or self._fresh:
            res = self._engine.refine(max_iters=self._refine_iters, eps=eps, fresh=self._fresh,
                                      reseed=self._reseed)[:3]
        return res


class MedianCutQuantizer(AbstractQuantizer):
    """Median cut on the MI355X engine (Engine.median_cut), optionally refined: the reference's
    MEDIAN_CUT (refine_iters = 0) and LBG_MEDIAN_CUT (refine_iters > 0) names.  getQuantizer keeps
    returning None for both, as the reference does."""

    def __init__(self, device=0, refine_iters=0, fresh=False, reseed=False):
        """refine_iters > 0 or fresh: Lloyd iterations warm-started from the median-cut codebook,
        stopped by eps (Engine.refine with C); reseed needs refine_iters > 0."""
        if reseed and int(refine_iters) <= 0:
            raise QVQError(1, "reseed needs refine_iters > 0")
        self._device = device
        self._engine = None
        self._refine_iters = int(refine_iters)
        self._fresh = bool(fresh)
        self._reseed = bool(reseed)

    def quantize(self, trainingSet, n, eps):
        if self._engine is None:
            self._engine = Engine(self._device)
        dev = getattr(trainingSet, "is_cuda", False)
        self._engine.set_vectors(trainingSet if dev else np.asarray(trainingSet, np.float64))
        res = self._engine.median_cut(int(n))[:3]
        if self._refine_iters > 0 or self._fresh:
            res = self._engine.refine(C=res[0], max_iters=self._refine_iters, eps=eps, fresh=self._fresh,
                                      reseed=self._reseed)[:3]
        return res


class KMeansPPQuantizer(AbstractQuantizer):
    """k-means++ seeding on the MI355X engine (Engine.kmeanspp) and Lloyd refinement from the seeds.
    The reference has no such quantizer and the Quantizers enum no slot for it."""

    def __init__(self, device=0, seed=0, refine_iters=0, fresh=False, reseed=False):
        """quantize seeds 2**n code vectors with `seed`, then runs Engine.refine from them for up to
        refine_iters iterations stopped by eps.  refine_iters = 0 returns the nearest-seed assignment
        (a fresh assignment with no iteration).  reseed needs refine_iters > 0."""
        if reseed and int(refine_iters) <= 0:
            raise QVQError(1, "reseed needs refine_iters > 0")
        self._device = device
        self._engine = None
        self._seed = int(seed)
        self._refine_iters = int(refine_iters)
        self._fresh = bool(fresh)
        self._reseed = bool(reseed)

    def quantize(self, trainingSet, n, eps):
        if self._engine is None:
            self._engine = Engine(self._device)
        dev = getattr(trainingSet, "is_cuda", False)
        self._engine.set_vectors(trainingSet if dev else np.asarray(trainingSet, np.float64))
        C = self._engine.kmeanspp(1 << int(n), self._seed)[0]
        return self._engine.refine(C=C, max_iters=self._refine_iters, eps=eps,
                                   fresh=self._fresh or self._refine_iters == 0, reseed=self._reseed)[:3]


class GreedyKMeansPPQuantizer(AbstractQuantizer):
    """Greedy k-means++ seeding on the MI355X engine (Engine.kmeanspp_greedy) and Lloyd refinement
    from the seeds.  The reference has no such quantizer and the Quantizers enum no slot for it."""

    def __init__(self, device=0, seed=0, trials=0, refine_iters=0, fresh=False, reseed=False):
        """quantize seeds 2**n code vectors with `seed`, `trials` candidate rows a round (0: the
        default count), then runs Engine.refine from them for up to refine_iters iterations stopped
        by eps.  refine_iters = 0 returns the nearest-seed assignment.  reseed needs refine_iters > 0."""
        if reseed and int(refine_iters) <= 0:
            raise QVQError(1, "reseed needs refine_iters > 0")
        if not 0 <= int(trials) <= 16:
            raise QVQError(1, "trials must be in 0 .. 16")
        self._device = device
        self._engine = None
        self._seed = int(seed)
        self._trials = int(trials)
        self._refine_iters = int(refine_iters)
        self._fresh = bool(fresh)
        self._reseed = bool(reseed)

    def quantize(self, trainingSet, n, eps):
        if self._engine is None:
            self._engine = Engine(self._device)
        dev = getattr(trainingSet, "is_cuda", False)
        self._engine.set_vectors(trainingSet if dev else np.asarray(trainingSet, np.float64))
        C = self._engine.kmeanspp_greedy(1 << int(n), self._seed, self._trials)[0]
        return self._engine.refine(C=C, max_iters=self._refine_iters, eps=eps,
                                   fresh=self._fresh or self._refine_iters == 0, reseed=self._reseed)[:3]


class KMeansParQuantizer(AbstractQuantizer):
    """k-means|| seeding on the MI355X engine (Engine.kmeans_par) and Lloyd refinement from the seeds.
    The reference has no such quantizer and the Quantizers enum no slot for it."""

    def __init__(self, device=0, seed=0, refine_iters=0, fresh=False, reseed=False, rounds=0, ell=0, round_cap=0):
        """quantize seeds 2**n code vectors with `seed` (rounds, ell, round_cap: Engine.kmeans_par's
        options, 0 the default), then runs Engine.refine from them for up to refine_iters iterations
        stopped by eps.  refine_iters = 0 returns the nearest-seed assignment (a fresh assignment with
        no iteration).  reseed needs refine_iters > 0."""
        if reseed and int(refine_iters) <= 0:
            raise QVQError(1, "reseed needs refine_iters > 0")
        self._device = device
        self._engine = None
        self._seed = int(seed)
        self._refine_iters = int(refine_iters)
        self._fresh = bool(fresh)
        self._reseed = bool(reseed)
        self._opts = (int(rounds), int(ell), int(round_cap))

    def quantize(self, trainingSet, n, eps):
        if self._engine is None:
            self._engine = Engine(self._device)
        dev = getattr(trainingSet, "is_cuda", False)
        self._engine.set_vectors(trainingSet if dev else np.asarray(trainingSet, np.float64))
        C = self._engine.kmeans_par(1 << int(n), self._seed, *self._opts)[0]
        return self._engine.refine(C=C, max_iters=self._refine_iters, eps=eps,
                                   fresh=self._fresh or self._refine_iters == 0, reseed=self._reseed)[:3]


def getQuantizer(q):
    """src/Quantizer.cpp:146-155: only LBG exists; other enumerators give None."""
    return LBGQuantizer() if Quantizers(q) == Quantizers.LBG else None
