"""The reference loop of qvq_refine (include/qvq.h) over the project's oracle, on the CPU:
oracle.kdtree_nn for the assignment, oracle.centroids(sum_mode=1) for the exact-sum centroids and
the direct sum for the distortion, under the entry's stop rules.  The yardstick of
tests/test_refine_cpu.py (against the committed trace) and tests/test_gpu_refine.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

STOP_FIXED, STOP_EPS, STOP_MAXIT = 0, 1, 2

# the three cases of tests/golden/refine_trace.json: (image side, block, bits)
CASES = {"s128_b2_6": (128, 2, 6), "s64_b2_4": (64, 2, 4), "s96_b4_5": (96, 4, 5)}


def distortion(X, C, A):
    """updateDistortion: the mean squared error of the rows against their code vectors."""
    return float(((X - C[A.astype(np.int64)]) ** 2).sum() / X.size)


def case_vectors(S, b, seed=0x5EED):
    rgb = oracle.gen_image(S, seed)
    X, _ = oracle.tile(rgb, S, S, b, b)
    return rgb, X


def lbg_start(X, bits):
    """What Engine.lbg returns: the reference rule's indices, the exact-sum
    centroids of their cells, the direct distortion of the two."""
    _, A, _ = oracle.lbg(X, bits, sum_mode=0)
    C = oracle.centroids(X, A, 1 << bits, sum_mode=1)
    return C, A, distortion(X, C, A)


def refine(X, C0, A0=None, d0=None, max_iters=100, eps=1e-6, fresh=False):
    """qvq_refine's contract: returns (C, A, distortion, info) with info = iters, stop, changed,
    distortion (the traces).  A0 / d0 None: a warm start (iteration 1 reports changed = N and
    takes no eps test)."""
    if max_iters == 0 and not fresh:
        raise ValueError("max_iters = 0 needs fresh")
    K = C0.shape[0]
    C, A, d = np.array(C0, np.float64), A0, d0
    changed, trace = [], []
    stop = STOP_MAXIT
    for t in range(1, max_iters + 1):
        A_t = oracle.kdtree_nn(C, X)
        C = oracle.centroids(X, A_t, K, sum_mode=1)
        d_t = distortion(X, C, A_t)
        n_chg = X.shape[0] if A is None else int((A_t != A).sum())
        changed.append(n_chg)
        trace.append(d_t)
        d_prev, A, d = d, A_t, d_t
        if n_chg == 0:
            stop = STOP_FIXED
            break
        if d_prev is not None and d_prev != 0 and abs(d_prev - d_t) / d_prev <= eps:
            stop = STOP_EPS
            break
    if fresh:
        A = oracle.kdtree_nn(C, X)
        d = distortion(X, C, A)
    return C, A, d, {"iters": len(changed), "stop": stop, "changed": changed, "distortion": trace}


def record():
    """The traces of CASES from the loop above (tests/golden/refine_trace.json)."""
    out = {}
    for name, (S, b, bits) in CASES.items():
        _, X = case_vectors(S, b)
        C0, A0, d0 = lbg_start(X, bits)
        _, _, d, info = refine(X, C0, A0, d0, max_iters=100, eps=0.0)
        A1 = oracle.kdtree_nn(C0, X)
        out[name] = {"S": S, "block": b, "bits": bits, "n": int(X.shape[0]), "iters": info["iters"],
                     "stop": info["stop"], "changed": info["changed"], "d_lbg": d0,
                     "d_reassign": distortion(X, C0, A1), "d_first": info["distortion"][0], "d_last": d}
    return out


if __name__ == "__main__":
    import json
    json.dump(record(), sys.stdout, indent=1)
    sys.stdout.write("\n")
