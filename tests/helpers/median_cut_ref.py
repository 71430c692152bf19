"""qvq_median_cut's contract (include/qvq.h) restated in numpy, for the device tests and the case
table.  It runs on the rows' ordinals u = (int8)code + 128, [N, dim] integers; the centroids come
from the oracle's exact-sum rule and the distortion is the direct sum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

NORMAL, SCALED = 0, 1


def ordinals_from_codes(codes):
    """u = (int8)b + 128 of code bytes."""
    return (np.asarray(codes, np.uint8).view(np.int8).astype(np.int64) + 128)


def codes_from_ordinals(u):
    return (np.asarray(u, np.int64) - 128).astype(np.int8).view(np.uint8)


def values(u, cs):
    """The fp64 rows of ordinals u under colour space cs: the space's table, which both spaces
    order by u (SCALED: fl(u * fl(1/255)); NORMAL: u - 128)."""
    tab = oracle.lut(cs)[codes_from_ordinals(np.arange(256))]
    assert np.all(np.diff(tab) > 0)
    return np.ascontiguousarray(tab[np.asarray(u, np.int64)])


def ordinals_from_values(X, cs):
    tab = oracle.lut(cs)[codes_from_ordinals(np.arange(256))]
    u = np.searchsorted(tab, X)
    assert np.array_equal(tab[u], X), "not a byte image of this colour space"
    return u


def axis_of(lo, hi):
    """The d with the largest hi - lo, the lowest on equal ranges; and that range."""
    r = np.asarray(hi, np.int64) - np.asarray(lo, np.int64)
    a = int(np.argmax(r))   # (numpy: the first maximum)
    return a, int(r[a])


def select(h, lo, hi, n):
    """t in [lo, hi - 1] minimising |2 cum(t) - n|, the lowest on ties; and the number of different
    splits (values of cum) that reach the minimum: 2 is a tie in the balance (empty bins repeat a
    split and do not count)."""
    cum = np.cumsum(np.asarray(h, np.int64))
    off = np.abs(2 * cum[lo:hi] - int(n))
    i = int(np.argmin(off))
    return lo + i, len(np.unique(cum[lo:hi][off == off[i]]))


def median_cut(u, bits):
    """(A uint32 [N], cuts [bits], trace): trace[l] lists level l + 1's boxes as dicts b, n, and for
    a cut box axis, lo, hi, t, ties (different splits that reach the balance's minimum), ranges (hi - lo per d)."""
    u = np.asarray(u, np.int64)
    N = u.shape[0]
    A = np.zeros(N, np.int64)
    cuts, trace = [], []
    for l in range(1, bits + 1):
        half = 1 << (l - 1)
        order = np.argsort(A, kind="stable")
        bounds = np.searchsorted(A[order], np.arange(half + 1))
        level, ncut = [], 0
        for b in range(half):
            rows = order[bounds[b]:bounds[b + 1]]
            n = len(rows)
            if n == 0:
                level.append({"b": b, "n": 0, "cut": False})
                continue
            lo, hi = u[rows].min(axis=0), u[rows].max(axis=0)
            ax, rng = axis_of(lo, hi)
            if rng == 0:
                level.append({"b": b, "n": n, "cut": False})
                continue
            h = np.bincount(u[rows, ax], minlength=256)
            t, ties = select(h, int(lo[ax]), int(hi[ax]), n)
            A[rows[u[rows, ax] > t]] = b + half
            ncut += 1
            level.append({"b": b, "n": n, "cut": True, "axis": ax, "lo": int(lo[ax]), "hi": int(hi[ax]), "t": t,
                          "ties": ties, "ranges": (hi - lo).tolist(), "at_t": int((u[rows, ax] == t).sum())})
        cuts.append(ncut)
        trace.append(level)
    return A.astype(np.uint32), cuts, trace


def distortion(X, C, A):
    """updateDistortion: the mean squared error of the rows against their code vectors."""
    return float(((X - C[A.astype(np.int64)]) ** 2).sum() / X.size)


def run(u, cs, bits):
    """What Engine.median_cut returns for the rows values(u, cs): (C, A, distortion, cuts)."""
    X = values(u, cs)
    A, cuts, _ = median_cut(u, bits)
    C = oracle.centroids(X, A, 1 << bits, sum_mode=1)
    return C, A, distortion(X, C, A), cuts
