"""qvq_kmeanspp's contract (include/qvq.h) restated in numpy and Python ints, for the device tests
and the case table.  It runs on the rows' ordinals o = code ^ 0x80, [N, dim] integers: pad
components are equal in every row and add nothing to a weight, so they are left out."""
import numpy as np

from helpers.median_cut_ref import NORMAL, SCALED, codes_from_ordinals, ordinals_from_values, values  # noqa: F401

MASK = (1 << 64) - 1
NO_ROW = 0xFFFFFFFF


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed, j, T):
    """floor(mix(seed + j) * T / 2^64), seed + j wrapping."""
    return (mix((int(seed) + int(j)) & MASK) * int(T)) >> 64


def weights(u, s):
    """w(row, s) for every row: exact int64."""
    d = u - u[s]
    return (d * d).sum(axis=1)


def kmeanspp(u, K, seed):
    """(rows uint32 [K], potential uint64 [K], placed, trace): trace[j - 1] describes draw j as a dict
    of T, t, s, boundary (t equals the prefix sum just before the drawn row, where > and >= part)
    and zero_before (the row before the drawn one has m = 0)."""
    u = np.asarray(u, np.int64)
    N = u.shape[0]
    rows, pot = np.full(K, NO_ROW, np.uint32), np.zeros(K, np.uint64)
    s = draw(seed, 0, N)
    m = weights(u, s)
    rows[0], pot[0] = s, int(m.sum())
    placed, trace = K, []
    for j in range(1, K):
        T = int(m.sum())
        if T == 0:
            placed = j
            break
        t = draw(seed, j, T)
        prefix = np.cumsum(m)   # (below 2^54: exact in int64)
        s = int(np.searchsorted(prefix, t, side="right"))   # the lowest row with prefix > t
        trace.append({"T": T, "t": t, "s": s, "boundary": s > 0 and int(prefix[s - 1]) == t,
                      "zero_before": s > 0 and int(m[s - 1]) == 0})
        m = np.minimum(m, weights(u, s))
        rows[j], pot[j] = s, int(m.sum())
    return rows, pot, placed, trace


def codebook(u, cs, rows, placed):
    """Entry j < placed the values of row rows[j] under colour space cs, the zero vector after."""
    u = np.asarray(u, np.int64)
    C = np.zeros((len(rows), u.shape[1]), np.float64)
    C[:placed] = values(u[rows[:placed].astype(np.int64)], cs)
    return C


def run(u, cs, K, seed):
    """What Engine.kmeanspp returns for the rows values(u, cs): (C, rows, potential, placed)."""
    rows, pot, placed, _ = kmeanspp(u, K, seed)
    return codebook(u, cs, rows, placed), rows, pot, placed


def brute_force(u, K, seed):
    """The rule again with nothing shared but mix: Python ints, every distance to every seed
    recomputed each round, a linear scan for the drawn row.  (rows, potential, placed) as lists."""
    u = [[int(v) for v in r] for r in np.asarray(u)]
    N = len(u)

    def w(a, b):
        return sum((x - y) ** 2 for x, y in zip(u[a], u[b]))

    seeds = [(mix((seed + 0) & MASK) * N) >> 64]
    pot = []
    while True:
        m = [min(w(r, s) for s in seeds) for r in range(N)]
        pot.append(sum(m))
        j = len(seeds)
        if j == K:
            return seeds, pot, K
        if pot[-1] == 0:
            return seeds, pot, j
        t = (mix((seed + j) & MASK) * pot[-1]) >> 64
        acc = 0
        for r in range(N):
            acc += m[r]
            if acc > t:
                seeds.append(r)
                break
