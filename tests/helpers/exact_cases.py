"""The cases the chunk, tile and grid edge tests of tests/test_gpu_exact.py run: exact mode
(qvq_set_vectors_exact, quant_amd/csrc/k_exact.hip) at the sizes where its kernels take another
path.  Plain data and the seeded, pure-numpy input builders; nothing here loads the
engine.

Every case names the qvq_exact_plan fields (include/qvq.h, quant_amd.host_exact_plan) it is there
for; tests/test_exact_plan.py checks them on the CPU, together with what each class claims about its
own inputs (which chunks win rows, which bands of the relative gap hold rows, which summation
mistakes the data shows) and the oracle's answers against the compiled reference kd-tree's recorded
ones (tests/golden/ref_nn_exact.json).

kc = 65536 / (8 D) code vectors fit the search's LDS chunk; T = 4096 / D rows fit a tile of the
Kahan chains.  kc_of and tile_rows_of below size the cases; the plan test checks both, for every D,
against what qvq_host_exact_plan derives from the engine's constants."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from helpers.shape_cases import row_bits  # noqa: E402

TIE_REL = 1e-12          # exact_assign's tie_rel (engine.cpp): rows within it go to the host kd-tree
TEMPLATED = (3, 6, 12, 48)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def gaussian_rows(N, D, seed):
    """tests/test_gpu_exact.py's generator: normal rows with a scale and an offset per column."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, D)) * rng.uniform(0.1, 10, size=D) + rng.uniform(-5, 5, size=D)


def wild_rows(N, D, seed):
    """lognormal(0, 4) with random signs: magnitudes over ~14 decades, so that almost every add of a
    sum rounds and a lost or restarted Kahan compensation shows in the result's bits."""
    rng = np.random.default_rng(seed)
    return rng.lognormal(0.0, 4.0, size=(N, D)) * rng.choice([-1.0, 1.0], size=(N, D))


def sqdist(X, C):
    """[N, K] squared distances in fp64, difference form (for ranks, not for bits)."""
    out = np.empty((len(X), len(C)))
    for i in range(0, len(X), 64):
        d = X[i:i + 64, None, :] - C[None]
        out[i:i + 64] = np.einsum("nkd,nkd->nk", d, d)
    return out


def best_two(X, C):
    """(i1, i2) per row: the nearest and the second nearest code vector by fp64 distance, the lower
    index first among equals."""
    o = np.argsort(sqdist(X, C), axis=1, kind="stable")[:, :2]
    return o[:, 0], o[:, 1]


# ---------------------------------------------------------------------------------------------
# (a) CHUNK_CASES, through qvq_assign: K at and around the multiples of kc, on the register-resident
# instantiations <3> <6> <12> <48> and on the generic one.
# ---------------------------------------------------------------------------------------------
CHUNK_N = 777             # three full 256-row blocks and nine rows
CHUNK_DS = (3, 6, 12, 48, 1, 5, 20, 33, 63, 64)
# K as a function of kc -> (chunks, last_chunk as a function of kc): the fields the case is there for
CHUNK_KS = {
    "kc": (lambda kc: kc, 1, lambda kc: kc),                  # LDS exactly full, the whole-codebook path
    "kc+1": (lambda kc: kc + 1, 2, lambda kc: 1),             # a chunk of one
    "2kc+1": (lambda kc: 2 * kc + 1, 3, lambda kc: 1),        # two full chunks and a chunk of one
}
CHUNK_KS_MORE = {                                             # D = 12 (templated) and D = 20 (generic) only
    "kc-1": (lambda kc: kc - 1, 1, lambda kc: kc - 1),
    "2kc": (lambda kc: 2 * kc, 2, lambda kc: kc),             # no partial chunk
    "3kc-7": (lambda kc: 3 * kc - 7, 3, lambda kc: kc - 7),   # a partial last chunk
}
N_DUP = 8                 # duplicated code vectors at k and k + kc (and one at k and K - 1)
# cases whose first seed fails a claim of tests/test_exact_plan.py (the kd-tree prefers the lower
# duplicate everywhere, or the last chunk's single code vector wins no row): key -> seeds to skip
CHUNK_RESEED = {
    "chunk-D3-Kkc+1": 2, "chunk-D3-K2kc+1": 7, "chunk-D12-Kkc+1": 2, "chunk-D1-Kkc+1": 3, "chunk-D1-K2kc+1": 2,
    "chunk-D20-Kkc+1": 2, "chunk-D20-K2kc+1": 4, "chunk-D33-Kkc+1": 1, "chunk-D63-Kkc+1": 2,
    "chunk-D63-K2kc+1": 2, "chunk-D64-Kkc+1": 3, "chunk-D64-K2kc+1": 1,
}


def kc_of(D):
    return 65536 // (8 * D)


def tile_rows_of(D):
    return 4096 // D


def _chunk_cases():
    out = []
    for D in CHUNK_DS:
        ks = dict(CHUNK_KS, **(CHUNK_KS_MORE if D in (12, 20) else {}))
        for name, (k_of, chunks, last_of) in ks.items():
            kc = kc_of(D)
            key = "chunk-D%d-K%s" % (D, name)
            out.append({"key": key, "D": D, "N": CHUNK_N, "K": k_of(kc), "K_name": name,
                        "seed": 7000 * D + k_of(kc) + 100000 * CHUNK_RESEED.get(key, 0),
                        "plan": {"kc": kc, "chunks": chunks, "last_chunk": last_of(kc),
                                 "templated": int(D in TEMPLATED)}})
    return out


CHUNK_CASES = _chunk_cases()


def build_chunk(D, K, seed):
    """(rows X [777, D], codebook C [K, D]).

    The code vectors, at random positions (so every chunk holds some of each kind):
      up to N / 4 exact copies of distinct rows (d1 = 0: the tie test's right side is 0);
      three zero vectors (equal code vectors far from the rows);
      the rest rows plus noise of 0.2 of the column's scale (near misses: a full scan decides).
    Then N_DUP exact copies, each of a different row, are duplicated from position k of the first
    chunk to k + kc (where K reaches), and one more to K - 1: the copied rows tie at distance 0
    between two chunks, so only the kd-tree's order of visit says which index the reference gives;
    with a last chunk of one code vector, that code vector is such a duplicate."""
    rng = np.random.default_rng(seed)
    kc = kc_of(D)
    X = gaussian_rows(CHUNK_N, D, seed)
    scale = X.std(axis=0)
    n_copy = min(K // 4, CHUNK_N // 4)
    copied = rng.choice(CHUNK_N, n_copy, replace=False)
    n_noise = K - n_copy - 3
    noisy = X[rng.integers(0, CHUNK_N, n_noise)] + rng.normal(size=(n_noise, D)) * 0.2 * scale
    C = np.concatenate([X[copied], np.zeros((3, D)), noisy])
    pos = rng.permutation(K)
    C = C[np.argsort(pos)]                                   # vector j of the list sits at position pos[j]
    first = np.sort(pos[:n_copy][pos[:n_copy] < min(kc, K - 1)])   # exact copies in the first chunk
    src = rng.choice(first, min(N_DUP + 1, len(first)), replace=False)
    for k in src[:-1]:
        for k2 in range(k + kc, K - 1, kc):
            C[k2] = C[k]
    C[K - 1] = C[src[-1]]
    return np.ascontiguousarray(X), np.ascontiguousarray(C)


# ---------------------------------------------------------------------------------------------
# (b) NEARTIE_CASES, through qvq_assign: pairs of code vectors on either side of tie_rel.
# ---------------------------------------------------------------------------------------------
EPS = (0.0, 1e-16, 1e-15, 1e-14, 1e-13, 3e-13, 1e-12, 3e-12, 1e-11, 1e-9, 1e-6)
DELTA0 = 2.0 ** -4                 # delta = DELTA0 * uniform(0.5, 2): far below the rows' spacing
# bands of the relative gap (d2 - d1) / d1, measured in long double from the stored fp64 inputs:
# (low, high] each, the first one the exact ties.  delta (1 + eps) makes the gap ~ 2 eps.
BANDS = ((-1.0, 0.0), (0.0, 1e-14), (1e-14, 1e-13), (1e-13, TIE_REL),
         (TIE_REL, 1e-10), (1e-10, 1e-8), (1e-8, np.inf))


def _neartie_cases():
    out = []
    for D in (12, 20):
        kc = kc_of(D)
        # kc + 1 is this table's own addition: in the chunk cases the code vector of a last chunk of one
        # is a duplicate, so its rows always go to the tree; here a row is decided there by the scan
        for name, K, chunks, last in (("kc", kc, 1, kc), ("kc+1", kc + 1, 2, 1), ("2kc+1", 2 * kc + 1, 3, 1)):
            for off in (0.0, 1e6):
                out.append({"key": "neartie-D%d-K%s-off%g" % (D, name, off), "D": D, "K": K, "N": K // 2,
                            "offset": off, "seed": 9000 * D + K + (17 if off else 0),
                            "plan": {"kc": kc, "chunks": chunks, "last_chunk": last,
                                     "templated": int(D in TEMPLATED)}})
    return out


NEARTIE_CASES = _neartie_cases()


def bands_expected(offset):
    """The bands a case at this data offset must fill.  A row's two differences delta and
    delta (1 + eps) are stored as multiples of ulp(offset), so at offset 1e6 a gap is either 0 --
    most of the small eps collapse to exact ties in the fp64 inputs, on purpose -- or at least one
    step, 2 ulp(offset) / delta_max: the bands wholly below that cannot hold a row."""
    if offset == 0:
        return list(BANDS)
    step = 2 * np.spacing(offset) / (2 * DELTA0)
    return [b for b in BANDS if b[1] <= 0 or b[1] > step]


def build_neartie(D, K, offset, seed):
    """(rows X [K // 2, D], codebook C [K, D], pair [K // 2, 2]).

    Row m has the code vectors b = x - delta (1 + eps) e_j at position pair[m, 0] and a = x + delta e_i
    at pair[m, 1] > pair[m, 0], eps cycling through EPS: the nearer vector always has the higher index,
    so a scan that prefers the lower of two near-equal distances, or a kd-tree answer where the fp64
    argmin is due, shows.  With more than one chunk every second pair has b in one chunk and a in
    the next; the others share a chunk.  A last chunk of one code vector is the nearer half of a
    pair with eps = 1e-6 (with K = kc + 1 the only pair across the boundary): that row's index comes
    from the scan of that chunk alone.  A slot no pair takes holds a vector 100 away from every row."""
    rng = np.random.default_rng(seed)
    kc, M = kc_of(D), K // 2
    X = gaussian_rows(M, D, seed) + offset
    chunks = [list(rng.permutation(np.arange(c0, min(c0 + kc, K)))) for c0 in range(0, K, kc)]
    pair = np.empty((M, 2), np.int64)
    m = 0
    nb, b, stalled = len(chunks) - 1, len(chunks) - 2, 0
    while m < M // 2 and stalled < nb:         # the straddling half, the last boundary served first
        if chunks[b] and chunks[b + 1]:
            pair[m] = chunks[b].pop(), chunks[b + 1].pop()
            m, stalled = m + 1, 0
        else:
            stalled += 1
        b = (b - 1) % nb
    for free in chunks:                        # the rest within a chunk
        while m < M and len(free) >= 2:
            pair[m] = sorted((free.pop(), free.pop()))
            m += 1
    assert m == M, "%d of %d pairs placed" % (m, M)
    pair = pair[rng.permutation(M)]
    last = np.flatnonzero(pair[:, 1] == K - 1)
    if len(chunks) > 1 and len(last):          # the chunk of one's pair: eps = 1e-6, no tie at any offset
        pair[[last[0], len(EPS) - 1]] = pair[[len(EPS) - 1, last[0]]]
    C = np.tile(X.mean(axis=0) + 100.0, (K, 1))
    delta = DELTA0 * rng.uniform(0.5, 2.0, M)
    ci, cj = rng.integers(0, D, M), rng.integers(0, D, M)
    for r in range(M):
        eps = EPS[r % len(EPS)]
        a, b = X[r].copy(), X[r].copy()
        a[ci[r]] += delta[r]
        b[cj[r]] -= delta[r] * (1 + eps)
        C[pair[r, 0]], C[pair[r, 1]] = b, a
    return np.ascontiguousarray(X), np.ascontiguousarray(C), pair


def pair_gap(X, C, pair):
    """Per row, in np.longdouble from the fp64 inputs as stored: the distances to its two code
    vectors (farther slot first, as pair) and the relative gap |d_b - d_a| / min."""
    x = X.astype(np.longdouble)
    d = [((x - C[pair[:, s]].astype(np.longdouble)) ** 2).sum(axis=1) for s in (0, 1)]
    lo = np.minimum(d[0], d[1])
    return d[0], d[1], np.abs(d[0] - d[1]) / lo


def band_counts(gap, bands=BANDS):
    return {b: int(np.sum((gap > b[0]) & (gap <= b[1]))) for b in bands}


# ---------------------------------------------------------------------------------------------
# (c) CHAIN_CASES, through qvq_update: one cell of every size around the unroll width (16) and
# the tile (T rows), on data that shows a wrong summation.
# ---------------------------------------------------------------------------------------------
CHAIN_DS = (1, 12, 33, 48, 63, 64)
# seeds to skip where a multi-tile cell's sum happens to survive one of the three mistakes
CHAIN_RESEED = {"chain-D1": 1393}     # one component: all four cells must show all three


def chain_sizes(T):
    return [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5]


CHAIN_CASES = [{"key": "chain-D%d" % D, "D": D, "K": len(chain_sizes(tile_rows_of(D))),
                "N": sum(chain_sizes(tile_rows_of(D))), "seed": 300 + D + 1000 * CHAIN_RESEED.get("chain-D%d" % D, 0),
                "plan": {"tile_rows": tile_rows_of(D)}} for D in CHAIN_DS]


def build_chain(D, seed):
    """(rows X, labels A): cell k has chain_sizes(T)[k] rows, dealt over the rows by a seeded
    permutation (the sorted order of the rows is not the identity)."""
    sizes = chain_sizes(tile_rows_of(D))
    rng = np.random.default_rng(seed)
    A = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)[rng.permutation(sum(sizes))]
    return wild_rows(sum(sizes), D, seed + 1), np.ascontiguousarray(A)


def kahan_mean(V, restart=0):
    """Kahan sum of V's rows in order times fl(1 / n), per column; restart > 0: the compensation
    starts again every `restart` rows (the mistake of a tile loop that does not carry it)."""
    s, c = np.zeros(V.shape[1]), np.zeros(V.shape[1])
    for i, v in enumerate(V):
        if restart and i % restart == 0:
            c = np.zeros(V.shape[1])
        y = v - c
        t = s + y
        c = (t - s) - y
        s = t
    return s * (1.0 / len(V))


def plain_mean(V):
    s = np.zeros(V.shape[1])
    for v in V:
        s = s + v
    return s * (1.0 / len(V))


# ---------------------------------------------------------------------------------------------
# (d) ROW_CASES and (e) MEAN_NS, through qvq_lbg: ragged row counts, more code vectors than rows,
# and the one-workgroup mean chain at its tile edges.
# ---------------------------------------------------------------------------------------------
ROW_NS = (1, 2, 3, 37, 255, 256, 257, 1025)
ROW_CASES = [{"key": "rows-D%d-N%d" % (D, N), "D": D, "N": N, "bits": row_bits(N), "seed": 40 * D + N}
             for D in (12, 5) for N in ROW_NS]

MEAN_D = 12


def mean_ns(T):
    return [1, 2, T - 1, T, T + 1, 2 * T + 1]


# bits = 0 returns the mean itself (the oracle and the engine both take it); bits = 1 its split
MEAN_CASES = [{"key": "mean-N%d-b%d" % (N, bits), "D": MEAN_D, "N": N, "bits": bits, "seed": 500 + N}
              for N in mean_ns(tile_rows_of(MEAN_D)) for bits in (0, 1)]

# (f) one case above every grid cap; (g) the same rows at 2^100 and 2^-100
STRIDE_CASE = {"key": "stride", "D": 3, "N": 2 ** 21 + 257, "bits": 3, "seed": 77}
SCALE_CASE = {"key": "scale", "D": 12, "N": 2000, "bits": 6, "seed": 88}
SCALES = (2.0 ** 100, 2.0 ** -100)


# ---------------------------------------------------------------------------------------------
# Inputs and oracle answers, built once per process and read-only
# ---------------------------------------------------------------------------------------------
_BY_KEY = {c["key"]: c for c in CHUNK_CASES + NEARTIE_CASES + CHAIN_CASES + ROW_CASES + MEAN_CASES +
           [STRIDE_CASE, SCALE_CASE]}
assert len(_BY_KEY) == (len(CHUNK_CASES) + len(NEARTIE_CASES) + len(CHAIN_CASES) + len(ROW_CASES) +
                        len(MEAN_CASES) + 2)


def key(c):
    return c["key"]


@functools.lru_cache(maxsize=None)
def _inputs(k):
    c = _BY_KEY[k]
    if k.startswith("chunk-"):
        return frozen(*build_chunk(c["D"], c["K"], c["seed"]))
    if k.startswith("neartie-"):
        return frozen(*build_neartie(c["D"], c["K"], c["offset"], c["seed"]))
    if k.startswith("chain-"):
        return frozen(*build_chain(c["D"], c["seed"]))
    if k.startswith("mean-"):
        return frozen(wild_rows(c["N"], c["D"], c["seed"]))
    return frozen(gaussian_rows(c["N"], c["D"], c["seed"]))


def inputs(c):
    """A case's inputs: (X, C) for (a), (X, C, pair) for (b), (X, A) for (c), X otherwise."""
    return _inputs(c["key"])


@functools.lru_cache(maxsize=None)
def _nn(k):
    X, C = _inputs(k)[:2]
    return frozen(oracle.kdtree_nn(C, X))


def oracle_nn(c):
    """oracle.kdtree_nn of an (a) or (b) case."""
    return _nn(c["key"])


@functools.lru_cache(maxsize=None)
def _lbg(k, scale):
    C, A, d = oracle.lbg(_inputs(k) * scale, _BY_KEY[k]["bits"], sum_mode=0)
    return frozen(C, A) + (d,)


def oracle_lbg(c, scale=1.0):
    """oracle.lbg(sum_mode=0) of a (d) ... (g) case: (C, A, distortion)."""
    return _lbg(c["key"], scale)
