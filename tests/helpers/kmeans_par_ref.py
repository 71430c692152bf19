"""qvq_kmeans_par's contract (include/qvq.h) restated in numpy and Python ints, for the device tests
and the case table.  It runs on the rows' ordinals o = code ^ 0x80, [N, dim] integers: pad
components are equal in every row and add nothing to a weight, so they are left out."""
import numpy as np

from helpers.kmeanspp_ref import MASK, NO_ROW, NORMAL, SCALED, codebook, draw, mix, ordinals_from_values, values  # noqa: F401

ROUNDS_MAX = 16
REDUCE_STREAM = 1 << 32


def options(K, rounds=0, ell=0, round_cap=0):
    """The options with the defaults filled in: (rounds, ell, round_cap, max_candidates)."""
    rounds = rounds or 5
    ell = ell or K
    round_cap = round_cap or 2 * ell + 64
    return rounds, ell, round_cap, 1 + rounds * round_cap


def mix_array(x):
    """mix over a uint64 array (numpy's unsigned arithmetic wraps)."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def mulhi_array(u, phi):
    """floor(u * phi / 2^64) for a uint64 array u and a Python int phi < 2^64, from 32-bit halves."""
    phi = int(phi)
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1 = u & m32, u >> s32
    b0, b1 = np.uint64(phi & 0xFFFFFFFF), np.uint64(phi >> 32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s32) + (p01 & m32) + (p10 & m32)
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def join_values(seed, r, N, phi):
    """mulhi64(u(r, row), phi) for every row, uint64 [N]."""
    key = mix((int(seed) + r) & MASK)
    with np.errstate(over="ignore"):
        u = mix_array(np.uint64(key) + np.arange(N, dtype=np.uint64))
        return mulhi_array(u, phi)


def weights_to(u, c):
    """w(row, c) for every row and every row index in c: int64 [N, len(c)]."""
    d = u[:, None, :] - u[None, np.asarray(c, np.int64), :]
    return (d * d).sum(axis=2)


def kmeans_par(u, K, seed, rounds=0, ell=0, round_cap=0):
    """The rule.  A dict of rows (uint32 [K]), cand_rows (uint32 [max_candidates]), cand_weights
    (uint64 [max_candidates]), info (as Engine.kmeans_par's) and trace: per round run a dict of phi,
    lhs (mulhi values), rhs (ell * m before the round), joined (all joining rows), kept, m_before; and
    near, m (final), picks (the seeds as candidate
    indices), reduction: the list of T per draw, max_product: the largest wt * g per draw."""
    u = np.asarray(u, np.int64)
    N = u.shape[0]
    rounds, ell, round_cap, max_c = options(K, rounds, ell, round_cap)
    cand = [draw(seed, 0, N)]
    m = weights_to(u, cand)[:, 0]
    near = np.zeros(N, np.int64)
    pot = [int(m.sum())]
    round_cand, truncated, rounds_run, trace = [0] * ROUNDS_MAX, 0, 0, []
    for r in range(1, rounds + 1):
        phi = int(m.sum())
        if phi == 0:
            break
        lhs = join_values(seed, r, N, phi)
        rhs = (ell * m).astype(np.uint64)
        joined = np.flatnonzero(lhs < rhs)
        kept = joined[:round_cap]
        truncated += len(joined) > round_cap
        m_before = m
        if len(kept):
            base = len(cand)
            step = max(1, (1 << 24) // (N * u.shape[1]))   # (bounded memory)
            for c0 in range(0, len(kept), step):
                w = weights_to(u, kept[c0:c0 + step])
                best = w.argmin(axis=1)   # the lowest index of the least weight
                wb = w[np.arange(N), best]
                take = wb < m
                near = np.where(take, base + c0 + best, near)
                m = np.where(take, wb, m)
            cand.extend(int(x) for x in kept)
        rounds_run = r
        round_cand[r - 1] = len(kept)
        pot.append(int(m.sum()))
        trace.append({"phi": phi, "lhs": lhs, "rhs": rhs, "joined": joined, "kept": kept, "m_before": m_before})
    M = len(cand)
    wt = np.bincount(near, minlength=M).astype(np.int64)
    cu = u[np.asarray(cand, np.int64)]
    # the reduction: Python ints for the products (below 2^54, the prefix exact in int64 as well)
    rows = np.full(K, NO_ROW, np.uint32)
    rs = (int(seed) + REDUCE_STREAM) & MASK
    s = int(np.searchsorted(np.cumsum(wt), draw(rs, 0, N), side="right"))
    picks, Ts, prods = [s], [], []
    d = cu - cu[s]
    g = (d * d).sum(axis=1)
    placed = K
    for j in range(1, K):
        prod = wt * g
        T = int(prod.sum())
        Ts.append(T)
        prods.append(int(prod.max()))
        if T == 0:
            placed = j
            break
        s = int(np.searchsorted(np.cumsum(prod), draw(rs, j, T), side="right"))
        picks.append(s)
        d = cu - cu[s]
        g = np.minimum(g, (d * d).sum(axis=1))
    rows[:len(picks)] = np.asarray(cand, np.int64)[picks]
    cand_rows = np.full(max_c, NO_ROW, np.uint32)
    cand_rows[:M] = cand
    cand_wt = np.zeros(max_c, np.uint64)
    cand_wt[:M] = wt
    info = {"placed": placed, "candidates": M, "rounds_run": rounds_run, "truncated": int(truncated),
            "round_candidates": round_cand, "potential": pot + [0] * (ROUNDS_MAX + 1 - len(pot))}
    return {"rows": rows, "cand_rows": cand_rows, "cand_weights": cand_wt, "info": info, "trace": trace,
            "near": near, "m": m, "picks": picks, "reduction": Ts, "max_product": prods}


def run(u, cs, K, seed, rounds=0, ell=0, round_cap=0):
    """What Engine.kmeans_par returns for the rows values(u, cs): (C, rows, cand_rows, cand_weights, info)."""
    out = kmeans_par(u, K, seed, rounds, ell, round_cap)
    return (codebook(u, cs, out["rows"], out["info"]["placed"]), out["rows"], out["cand_rows"], out["cand_weights"],
            out["info"])


def brute_force(u, K, seed, rounds=0, ell=0, round_cap=0):
    """The rule again with nothing shared but mix: Python ints, every weight to every candidate
    recomputed, linear scans.  (rows, cand_rows, cand_weights, placed, potential, truncated) as lists,
    without the padding past M and placed."""
    u = [[int(v) for v in r] for r in np.asarray(u)]
    N = len(u)
    rounds = rounds or 5
    ell = ell or K
    round_cap = round_cap or 2 * ell + 64

    def w(a, b):
        return sum((x - y) ** 2 for x, y in zip(u[a], u[b]))

    def nearest(row, cand):
        best, arg = None, None
        for i, c in enumerate(cand):
            v = w(row, c)
            if best is None or v < best:
                best, arg = v, i
        return best, arg

    cand = [(mix(seed & MASK) * N) >> 64]
    pot, truncated = [], 0
    for r in range(1, rounds + 1):
        m = [nearest(row, cand)[0] for row in range(N)]
        phi = sum(m)
        pot.append(phi)
        if phi == 0:
            break
        key = mix((seed + r) & MASK)
        joined = [row for row in range(N) if (mix((key + row) & MASK) * phi) >> 64 < ell * m[row]]
        truncated += len(joined) > round_cap
        cand += joined[:round_cap]
    else:
        pot.append(sum(nearest(row, cand)[0] for row in range(N)))
    wt = [0] * len(cand)
    for row in range(N):
        wt[nearest(row, cand)[1]] += 1
    rs = (seed + (1 << 32)) & MASK
    picks = []
    for j in range(K):
        if j == 0:
            val, T = wt, N
        else:
            val = [wt[c] * min(w(cand[c], cand[s]) for s in picks) for c in range(len(cand))]
            T = sum(val)
            if T == 0:
                break
        t = (mix((rs + j) & MASK) * T) >> 64
        acc = 0
        for c, v in enumerate(val):
            acc += v
            if acc > t:
                picks.append(c)
                break
    return [cand[c] for c in picks], cand, wt, len(picks), pot, truncated
