"""qvq_kmeanspp_greedy's contract (include/qvq.h) restated in numpy and Python ints, for the device
tests and the case table.  The terms are kmeanspp_ref's: the rows' ordinals o = code ^ 0x80 as [N, dim]
integers (pad components add nothing to a weight and are left out), mix, draw and the weights."""
import numpy as np

from helpers.kmeanspp_ref import MASK, NO_ROW, NORMAL, SCALED, codebook, draw, mix, values, weights  # noqa: F401
from helpers.kmeanspp_ref import ordinals_from_values  # noqa: F401

MAX_TRIALS = 16
NO_TRIAL = 0xFFFFFFFF


def trials(K, trials=0):
    """L: trials itself, or for 0 the default 2 + 7 floor(log2 K) / 10."""
    K, trials = int(K), int(trials)
    if not (1 <= K <= 1 << 20 and 0 <= trials <= MAX_TRIALS):
        raise ValueError("K must be in 1 .. 2^20 and trials in 0 .. 16")
    return trials if trials else 2 + 7 * (K.bit_length() - 1) // 10


def trial_seed(seed, l):
    """The stream of trial l: seed + l 2^32, wrapping."""
    return (int(seed) + (int(l) << 32)) & MASK


def kmeanspp_greedy(u, K, seed, n_trials=0):
    """A dict of rows uint32 [K], potential uint64 [K], placed, trials (L), trial uint32 [K],
    trial_rows uint32 [K, 16], trial_potential uint64 [K, 16] and trace: trace[j - 1] describes round
    j as a dict of T and per trial the lists t, c, P, boundary (t equals the prefix sum just before
    the drawn row) and zero_before (the row before the drawn one has m = 0)."""
    u = np.asarray(u, np.int64)
    N = u.shape[0]
    L = trials(K, n_trials)
    rows, pot = np.full(K, NO_ROW, np.uint32), np.zeros(K, np.uint64)
    trial = np.full(K, NO_TRIAL, np.uint32)
    trows, tpot = np.full((K, MAX_TRIALS), NO_ROW, np.uint32), np.zeros((K, MAX_TRIALS), np.uint64)
    s = draw(seed, 0, N)
    m = weights(u, s)
    rows[0], pot[0], trial[0] = s, int(m.sum()), 0
    trows[0, 0], tpot[0, 0] = s, pot[0]
    placed, trace = K, []
    for j in range(1, K):
        T = int(m.sum())
        if T == 0:
            placed = j
            break
        prefix = np.cumsum(m)   # (below 2^54: exact in int64)
        rec = {"T": T, "t": [], "c": [], "P": [], "boundary": [], "zero_before": []}
        best = None
        for l in range(L):
            t = draw(trial_seed(seed, l), j, T)
            c = int(np.searchsorted(prefix, t, side="right"))   # the lowest row with prefix > t
            cand = np.minimum(m, weights(u, c))
            P = int(cand.sum())
            rec["t"].append(t), rec["c"].append(c), rec["P"].append(P)
            rec["boundary"].append(c > 0 and int(prefix[c - 1]) == t)
            rec["zero_before"].append(c > 0 and int(m[c - 1]) == 0)
            trows[j, l], tpot[j, l] = c, P
            if best is None or P < best[0]:   # strict: the lowest l wins a tie
                best = (P, l, cand)
        trace.append(rec)
        pot[j], trial[j], m = best
        rows[j] = rec["c"][best[1]]
    return {"rows": rows, "potential": pot, "placed": placed, "trials": L, "trial": trial, "trial_rows": trows,
            "trial_potential": tpot, "trace": trace}


def run(u, cs, K, seed, n_trials=0):
    """What Engine.kmeanspp_greedy returns for the rows values(u, cs): (C, rows, potential, info)."""
    r = kmeanspp_greedy(u, K, seed, n_trials)
    info = {k: r[k] for k in ("placed", "trials", "trial", "trial_rows", "trial_potential")}
    return codebook(u, cs, r["rows"], r["placed"]), r["rows"], r["potential"], info


def brute_force(u, K, seed, L):
    """The rule again with nothing shared but mix: Python ints, every distance to every seed
    recomputed each round, linear scans for the drawn rows.  (rows, potential, placed, trial,
    trial_rows, trial_potential) as lists, the last two with L entries per published round."""
    u = [[int(v) for v in r] for r in np.asarray(u)]
    N = len(u)

    def w(a, b):
        return sum((x - y) ** 2 for x, y in zip(u[a], u[b]))

    def near(seeds):
        return [min(w(r, s) for s in seeds) for r in range(N)]

    seeds = [(mix(seed & MASK) * N) >> 64]
    pot, trial, trows, tpot = [sum(near(seeds))], [0], [[seeds[0]]], [[sum(near(seeds))]]
    while True:
        j = len(seeds)
        if j == K:
            return seeds, pot, K, trial, trows, tpot
        m = near(seeds)
        if sum(m) == 0:
            return seeds, pot, j, trial, trows, tpot
        cs, Ps = [], []
        for l in range(L):
            t = (mix((seed + (l << 32) + j) & MASK) * sum(m)) >> 64
            acc = 0
            for r in range(N):
                acc += m[r]
                if acc > t:
                    cs.append(r)
                    break
            Ps.append(sum(near(seeds + [cs[-1]])))
        win = Ps.index(min(Ps))
        seeds.append(cs[win])
        pot.append(Ps[win]), trial.append(win), trows.append(cs), tpot.append(Ps)
