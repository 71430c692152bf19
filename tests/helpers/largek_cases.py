"""The cases of tests/test_gpu_largek.py: codebooks past each kernel's LDS capacity, where the
dispatch leaves the benchmark shapes' kernels for tiled loops, chunked sweeps, several passes or
host paths.  Plain data and the input builders; nothing here loads the engine.

Every case names the qvq_plan fields (include/qvq.h, quant_amd.host_plan) it is there for.
tests/test_largek_plan.py checks on the CPU that the engine's own dispatch predicates still give
those values, and that the table as a whole reaches every path.  The thresholds live in this table
only: when a kernel's capacity moves, that test names the case that no longer covers its path, and
the case moves with the threshold.

Field values are written as in qvq.h: search small | mf32 | wide | valu, recheck mf32 | staged |
chunked | global, update runs | sorted | lds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

# side of the square raster per block shape (bw, bh): at most 16384 rows each
SIDE = {(2, 2): 256, (4, 4): 256, (3, 3): 192, (1, 1): 128, (2, 3): 96}


def dim(bw, bh):
    return 3 * bw * bh


def rows(bw, bh, S=None):
    S = S or SIDE[(bw, bh)]
    return ((S + bw - 1) // bw) * ((S + bh - 1) // bh)


# ---------------------------------------------------------------------------------------------
# (a) qvq_assign.  plan: the default dispatch; valu: the dispatch under QVQ_SEARCH=valu (run for
# every D != 12; at D = 12 the VALU search is the default past mf_can_search).
# ---------------------------------------------------------------------------------------------
def _a(bw, bh, K, plan, valu=None):
    return {"bw": bw, "bh": bh, "K": K, "plan": plan, "valu": valu}


ASSIGN_CASES = [
    # D = 12 (2x2)
    _a(2, 2, 1025, {"search": "mf32", "fused": 0, "c32_staged": 1, "recheck": "mf32", "prune": 1}),
    _a(2, 2, 1568, {"search": "mf32", "c32_staged": 1}),            # last K with the fp32 codebook in LDS
    _a(2, 2, 1569, {"search": "mf32", "c32_staged": 0}),
    _a(2, 2, 1632, {"recheck": "mf32"}),                            # last K of the MFMA recheck
    _a(2, 2, 1633, {"recheck": "staged", "search": "mf32"}),
    _a(2, 2, 2048, {"prune": 1, "search": "mf32"}),                 # last pruned level
    _a(2, 2, 2912, {"search": "mf32", "prune": 0, "recheck": "staged"}),   # last K of the MFMA search
    _a(2, 2, 2913, {"search": "valu", "valu_tiles": 3, "recheck": "staged"}),
    _a(2, 2, 3114, {"search": "valu", "recheck": "staged"}),        # last K staged whole by the recheck
    _a(2, 2, 3115, {"search": "valu", "recheck": "chunked"}),
    _a(2, 2, 4096, {"recheck": "chunked", "device_tree": 1, "valu_tiles": 4}),
    _a(2, 2, 4097, {"recheck": "chunked", "device_tree": 0, "valu_tiles": 4}),
    _a(2, 2, 8192, {"search": "valu", "valu_tiles": 7, "recheck": "chunked"}),
    _a(2, 2, 16385, {"search": "valu", "valu_tiles": 13, "recheck": "chunked", "update": "lds"}),
    # D = 48 (4x4)
    _a(4, 4, 718, {"search": "wide", "cb_resident": 0, "recheck": "staged"}, {"valu_tiles": 3, "recheck": "staged"}),
    _a(4, 4, 719, {"search": "wide", "recheck": "chunked"}, {"valu_tiles": 3, "recheck": "chunked"}),
    _a(4, 4, 4097, {"search": "wide", "recheck": "chunked", "prune": 0, "device_tree": 0},
       {"valu_tiles": 13, "recheck": "chunked"}),
    _a(4, 4, 8192, {"search": "wide", "cb_resident": 0, "recheck": "chunked"}, {"valu_tiles": 25}),
    # D = 27 (3x3), rows padded to 28
    _a(3, 3, 1334, {"search": "wide", "recheck": "staged"}, {"valu_tiles": 3, "recheck": "staged"}),
    _a(3, 3, 1335, {"search": "wide", "recheck": "global"}, {"valu_tiles": 3, "recheck": "global"}),
    _a(3, 3, 2048, {"search": "wide", "cb_resident": 0, "recheck": "global", "prune": 1},
       {"valu_tiles": 4, "recheck": "global"}),
    # D = 3 (1x1), rows padded to 4
    _a(1, 1, 2048, {"search": "wide", "cb_resident": 1, "recheck": "staged"}, {"valu_tiles": 1}),
    _a(1, 1, 2049, {"search": "wide", "cb_resident": 0, "recheck": "staged"}, {"valu_tiles": 1}),
    _a(1, 1, 9344, {"search": "wide", "recheck": "staged"}, {"valu_tiles": 3, "recheck": "staged"}),
    _a(1, 1, 9345, {"search": "wide", "recheck": "global"}, {"valu_tiles": 3, "recheck": "global"}),
    _a(1, 1, 16384, {"search": "wide", "cb_resident": 0, "recheck": "global"}, {"valu_tiles": 5}),
    # D = 18 (2x3), rows padded to 20
    _a(2, 3, 2000, {"search": "wide", "cb_resident": 0, "recheck": "global"},
       {"valu_tiles": 3, "recheck": "global"}),
]


def assign_vectors(bw, bh):
    """The training set of an assign case: the synthetic image tiled bw x bh."""
    S = SIDE[(bw, bh)]
    X, _ = oracle.tile(oracle.gen_image(S), S, S, bw, bh)
    return X


def codebook(X, K, seed):
    """K code vectors over the rows X: split pairs base * 1.2 | base * 0.8 (near ties: flagged rows),
    four zero vectors, and base[:4] twice (the rows equal to one of them tie exactly between the two
    copies), cut to K -- at least three of the duplicate pairs survive the cut."""
    rng = np.random.default_rng(seed)
    n = (K - 12 + 1) // 2
    base = X[rng.choice(len(X), n, replace=True)]
    C = np.concatenate([base * (1 + 0.2), base * (1 - 0.2), np.zeros((4, X.shape[1])), base[:4], base[:4]])[:K]
    assert C.shape[0] == K
    return np.ascontiguousarray(C)


# ---------------------------------------------------------------------------------------------
# (b) qvq_update.
# ---------------------------------------------------------------------------------------------
def _u(bw, bh, K, plan, n=None):
    return {"bw": bw, "bh": bh, "K": K, "plan": plan, "n": n}


UPDATE_CASES = [
    _u(2, 2, 1, {"update": "runs", "update_copies": 16}),
    _u(2, 2, 40, {"update": "runs", "update_copies": 16}),
    _u(2, 2, 100, {"update": "runs", "update_copies": 8}),
    _u(2, 2, 127, {"update": "runs", "update_copies": 4}),       # K * D = 1524: last K of the runs
    _u(2, 2, 128, {"update": "sorted"}),                         # K * D = 1536
    _u(4, 4, 31, {"update": "runs", "update_copies": 4}),
    _u(4, 4, 32, {"update": "sorted"}),
    _u(1, 1, 500, {"update": "runs", "update_copies": 4}),
    _u(3, 3, 56, {"update": "runs", "update_copies": 4}),
    _u(3, 3, 57, {"update": "sorted"}),
    _u(2, 2, 16384, {"update": "sorted"}),                       # last K of the counting sort
    _u(2, 2, 16385, {"update": "lds", "update_copies": 11}),     # 11 passes of KR = 1515, the last of 1235
    _u(2, 2, 20000, {"update": "lds", "update_copies": 14}),     # the last pass of 305
    _u(4, 4, 16385, {"update": "lds", "update_copies": 43}),
    _u(1, 1, 32768, {"update": "lds", "update_copies": 7}),
]

# The dispatch alone, no GPU run: update_runs_kernel with one copy of the sums is what launch_update
# picks only when the counting sort is out (2^32 rows or more) and K * D is past the replicas' room;
# the engine takes no training set of that many rows, so nothing can run this shape.
PLAN_ONLY_CASES = [
    _u(2, 2, 1000, {"update": "runs", "update_copies": 1}, n=1 << 32),
]


def update_vectors(bw, bh):
    """(raster, rows X) of an update case: a noise raster tiled bw x bh."""
    S = SIDE[(bw, bh)]
    rgb = noise(S, seed=5)
    X, _ = oracle.tile(rgb, S, S, bw, bh)
    return rgb, S, X


def assignments(N, K, seed):
    """The three assignments of an update case."""
    rng = np.random.default_rng(seed)
    used = max(1, K - max(1, K // 10)) if K > 1 else 1
    # a tenth of the cells, anywhere in the range, stay empty: every pass of KR cells keeps live ones
    live = np.sort(rng.permutation(K)[:used]).astype(np.uint32)
    return {
        "uniform": live[rng.integers(0, used, N)],
        # long runs of one index: the run accumulators flush on an index change, not on every row
        "blocky": live[(np.arange(N, dtype=np.uint64) * np.uint64(used)) // np.uint64(N)],
        # every row in the last code vector of the last pass
        "last": np.full(N, K - 1, np.uint32),
    }


# ---------------------------------------------------------------------------------------------
# (c) qvq_lbg.  levels: {K: fields} of the levels the case is there for.
# ---------------------------------------------------------------------------------------------
def _l(name, S, bw, bh, bits, levels, cs="scaled"):
    return {"name": name, "S": S, "bw": bw, "bh": bh, "bits": bits, "cs": cs, "levels": levels}


LBG_CASES = [
    _l("2x2_n11", 256, 2, 2, 11, {32: {"search": "small", "fused": 1},
                                  1024: {"search": "mf32", "fused": 1, "prune": 1},
                                  2048: {"search": "mf32", "fused": 0, "prune": 1, "c32_staged": 0,
                                         "recheck": "staged", "update": "sorted"}}),
    _l("2x2_n12", 256, 2, 2, 12, {4096: {"search": "valu", "valu_tiles": 4, "prune": 0, "recheck": "chunked"}}),
    _l("2x2_n13", 256, 2, 2, 13, {8192: {"search": "valu", "valu_tiles": 7, "device_tree": 0, "update": "sorted"}}),
    _l("2x2_n15_more_cells_than_rows", 128, 2, 2, 15, {16384: {"update": "sorted"},
                                                       32768: {"search": "valu", "update": "lds",
                                                               "update_copies": 22}}),
    _l("3x3_n11", 192, 3, 3, 11, {2048: {"search": "wide", "prune": 1, "recheck": "global"}}),
    _l("3x3_n13", 192, 3, 3, 13, {8192: {"search": "wide", "prune": 0, "recheck": "global"}}),
    _l("4x4_n13", 256, 4, 4, 13, {4096: {"search": "wide", "prune": 1, "device_tree": 1},
                                  8192: {"search": "wide", "prune": 0, "device_tree": 0, "recheck": "chunked"}}),
    _l("1x1_n14", 128, 1, 1, 14, {2048: {"cb_resident": 1, "prune": 0},
                                  4096: {"cb_resident": 0, "prune": 1},
                                  16384: {"search": "wide", "recheck": "global", "update": "sorted"}}),
    _l("2x2_n12_normal", 256, 2, 2, 12, {4096: {"search": "valu"}}, cs="normal"),
]


def noise(S, seed=1):
    """S x S RGB noise raster (as tests/test_gpu_prune.py _image("noise"))."""
    return np.random.default_rng(seed).integers(0, 256, size=S * S * 3, dtype=np.uint8)
