"""qvq_lbg_lloyd's rule (include/qvq.h) restated over the project's oracle, on the CPU: the mean,
then per level the split as two numpy products and qvq_refine's loop as tests/helpers/refine_ref.py
(or, with the flag, reseed_ref.py) restates it, warm-started from the split.  The yardstick of
tests/test_lbg_lloyd_cpu.py (against the committed trace) and tests/test_gpu_lbg_lloyd.py."""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import oracle  # noqa: E402
from helpers import refine_ref, reseed_ref  # noqa: E402
from helpers.lbg_lloyd_cases import CASES, NORMAL, SCALED  # noqa: E402,F401
from helpers.refine_ref import STOP_FIXED, STOP_EPS, STOP_MAXIT, distortion  # noqa: E402,F401

LEVEL_FIELDS = ("iters", "stop", "changed", "empty", "seeds", "distortion")


def vectors(rgb, xs, ys, bw, bh, cs):
    """The rows of a raster under colour space cs."""
    return oracle.tile(rgb, xs, ys, bw, bh, cs, 128 if cs == SCALED else 0)[0]


def case_vectors(name):
    c = CASES[name]
    return vectors(oracle.gen_image(c.S), c.S, c.S, c.block, c.block, c.cs)


def mean(X):
    """C^(0): the exact sum of the rows rounded once, times fl(1/N) (qvq_lbg's first code vector)."""
    return oracle.centroids(X, np.zeros(X.shape[0], np.uint32), 1, sum_mode=1)


def split(C):
    """S[k] = C[k] (1 + 0.2), S[k + H] = C[k] (1 - 0.2): fp64 products."""
    return np.concatenate([C * (1 + 0.2), C * (1 - 0.2)])


def lbg_lloyd(X, bits, iters, eps=1e-6, cs=SCALED, reseed=False, on_level=None):
    """(C, A, d, levels): levels[l] = iters, stop, changed, empty, seeds, distortion of level l + 1.
    on_level(l, S, info): called with every level's split and loop info (the eps-margin test)."""
    if iters < 1:
        raise ValueError("iters must be >= 1")
    C = mean(X)
    A = np.zeros(X.shape[0], np.uint32)
    d = distortion(X, C, A)
    levels = []
    for l in range(1, bits + 1):
        S = split(C)
        if reseed:
            C, A, d, info = reseed_ref.refine(X, S, cs, max_iters=iters, eps=eps)
        else:
            C, A, d, info = refine_ref.refine(X, S, max_iters=iters, eps=eps)
        if on_level:
            on_level(l, S, info)
        levels.append({"iters": info["iters"], "stop": info["stop"], "changed": info["changed"][-1],
                       "empty": reseed_ref.empty_cells(A, C.shape[0]), "seeds": sum(info.get("reseeded", [])),
                       "distortion": d})
    return C, A, d, levels


def continue_refine(X, run, cs, max_iters, eps=0.0, reseed=False):
    """qvq_refine(C_start = NULL) after the run (C, A, d, levels)."""
    C, A, d, _ = run
    if reseed:
        return reseed_ref.refine(X, C, cs, A, d, max_iters=max_iters, eps=eps)
    return refine_ref.refine(X, C, A, d, max_iters=max_iters, eps=eps)


_RUNS = {}


def run_case(name):
    """(X, lbg_lloyd(...)) of a case of the table, computed once per process."""
    if name not in _RUNS:
        c = CASES[name]
        X = case_vectors(name)
        _RUNS[name] = (X, lbg_lloyd(X, c.bits, c.iters, c.eps, c.cs, c.reseed))
    return _RUNS[name]


TRACE_PATH = os.path.join(TESTS, "golden", "lbg_lloyd_trace.json")


def record(path=TRACE_PATH):
    """Every level of every case, written to tests/golden/lbg_lloyd_trace.json."""
    import json
    out = {}
    for name, c in CASES.items():
        X, (_, _, d, levels) = run_case(name)
        out[name] = dict(c._asdict(), n=int(X.shape[0]), d_last=d, levels=levels)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    record()
