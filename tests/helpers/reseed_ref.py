"""The reseed rule of qvq_refine's QVQ_REFINE_RESEED (include/qvq.h) restated in numpy over the
project's oracle, on the CPU: refine_ref.refine's loop with the empty cells of each iteration's
centroids seeded from the worst cells.  The per-row error is a Python loop over the components, so
its order is the contract's and not numpy's pairwise sum.  The yardstick of
tests/test_reseed_cpu.py (against the committed trace) and tests/test_gpu_reseed.py."""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import oracle  # noqa: E402
from helpers import refine_ref  # noqa: E402
from helpers.refine_ref import STOP_FIXED, STOP_EPS, STOP_MAXIT, distortion  # noqa: E402,F401

NORMAL, SCALED = 0, 1
SHIFT = {SCALED: 24, NORMAL: 8}

# (image side, block, bits, colour space): refine_ref.CASES in both spaces, and the 10-bit codebook
CASES = {
    "s128_b2_6_scaled": (128, 2, 6, SCALED), "s128_b2_6_normal": (128, 2, 6, NORMAL),
    "s96_b4_5_scaled": (96, 4, 5, SCALED),
    "s64_b2_4_scaled": (64, 2, 4, SCALED), "s64_b2_4_normal": (64, 2, 4, NORMAL),
    "s128_b2_10_scaled": (128, 2, 10, SCALED), "s128_b2_10_normal": (128, 2, 10, NORMAL),
}


def case_vectors(S, b, cs, seed=0x5EED):
    """(rgb, X): X the rows under colour space cs."""
    rgb = oracle.gen_image(S, seed)
    X, _ = oracle.tile(rgb, S, S, b, b, cs, 128 if cs == SCALED else 0)
    return rgb, X


def row_errors(X, C, A, cs):
    """q_row = floor(e 2^s), e the sum of (x_d - C[A[row]][d])^2 over d ascending, each operation
    rounded once (numpy element-wise operations on float64 columns are)."""
    c = C[A.astype(np.int64)]
    e = np.zeros(X.shape[0], np.float64)
    for d in range(X.shape[1]):
        u = X[:, d] - c[:, d]
        e = e + u * u
    return np.floor(e * float(1 << SHIFT[cs])).astype(np.uint64)


def cell_stats(q, A, K):
    """(E, n, far): the cells' summed errors, rows, and far rows (-1: no row)."""
    E = np.zeros(K, np.uint64)
    n = np.zeros(K, np.uint64)
    far = np.full(K, -1, np.int64)
    best = np.zeros(K, np.uint64)
    for row in range(len(A)):
        k = int(A[row])
        E[k] += q[row]
        n[k] += np.uint64(1)
        if far[k] < 0 or q[row] > best[k]:   # (equal q: the lower row stays)
            far[k], best[k] = row, q[row]
    return E, n, far


def select(E, n):
    """(empties, donors): empties ascending; donors (n >= 2, E > 0) by E descending, then k
    ascending; both cut to m = min of the two."""
    K = len(E)
    empties = [k for k in range(K) if n[k] == 0]
    donors = sorted((k for k in range(K) if n[k] >= 2 and E[k] > 0), key=lambda k: (-int(E[k]), k))
    m = min(len(empties), len(donors))
    return empties[:m], donors[:m]


def reseed(X, C, A, cs):
    """C with its seeds (a copy) and the number placed."""
    K = C.shape[0]
    n = np.bincount(A.astype(np.int64), minlength=K)
    if not (n == 0).any():
        return C, 0
    E, n64, far = cell_stats(row_errors(X, C, A, cs), A, K)
    empties, donors = select(E, n64)
    C = C.copy()
    for e, dn in zip(empties, donors):
        C[e] = X[far[dn]]
    return C, len(empties)


def refine(X, C0, cs, A0=None, d0=None, max_iters=100, eps=1e-6, fresh=False):
    """qvq_refine's contract with QVQ_REFINE_RESEED: refine_ref.refine plus info["reseeded"]."""
    if max_iters == 0 and not fresh:
        raise ValueError("max_iters = 0 needs fresh")
    K = C0.shape[0]
    C, A, d = np.array(C0, np.float64), A0, d0
    changed, trace, seeds = [], [], []
    stop = STOP_MAXIT
    for t in range(1, max_iters + 1):
        A_t = oracle.kdtree_nn(C, X)
        C = oracle.centroids(X, A_t, K, sum_mode=1)
        d_t = distortion(X, C, A_t)
        C, m = reseed(X, C, A_t, cs)
        n_chg = X.shape[0] if A is None else int((A_t != A).sum())
        changed.append(n_chg)
        trace.append(d_t)
        seeds.append(m)
        d_prev, A, d = d, A_t, d_t
        if n_chg == 0 and m == 0:
            stop = STOP_FIXED
            break
        if d_prev is not None and d_prev != 0 and abs(d_prev - d_t) / d_prev <= eps:
            stop = STOP_EPS
            break
    if fresh:
        A = oracle.kdtree_nn(C, X)
        d = distortion(X, C, A)
    return C, A, d, {"iters": len(changed), "stop": stop, "changed": changed, "distortion": trace,
                     "reseeded": seeds}


def lbg_start(X, bits):
    return refine_ref.lbg_start(X, bits)


def empty_cells(A, K):
    return int((np.bincount(A.astype(np.int64), minlength=K) == 0).sum())


_RUNS = {}


def run_case(name, max_iters=100):
    """(X, (C0, A0, d0), refine(...) with eps = 0) of a case, computed once per process."""
    key = (name, max_iters)
    if key not in _RUNS:
        S, b, bits, cs = CASES[name]
        _, X = case_vectors(S, b, cs)
        start = lbg_start(X, bits)
        _RUNS[key] = (X, start, refine(X, start[0], cs, start[1], start[2], max_iters=max_iters, eps=0.0))
    return _RUNS[key]


def record():
    """The traces of CASES (tests/golden/refine_reseed_trace.json); the 10-bit cases run 6 iterations."""
    out = {}
    for name, (S, b, bits, cs) in CASES.items():
        iters = 6 if bits == 10 else 100
        X, (C0, A0, d0), (C, A, d, info) = run_case(name, iters)
        out[name] = {"S": S, "block": b, "bits": bits, "colorspace": cs, "n": int(X.shape[0]), "max_iters": iters,
                     "iters": info["iters"], "stop": info["stop"], "changed": info["changed"],
                     "reseeded": info["reseeded"], "distortion": info["distortion"], "d_lbg": d0, "d_last": d,
                     "empty_last": empty_cells(A, C.shape[0])}
    return out


if __name__ == "__main__":
    import json
    json.dump(record(), sys.stdout, indent=1)
    sys.stdout.write("\n")
