"""The cases of tests/test_gpu_prune_bound.py: codebooks on which the pruned
searches' projection bound ||x - c||^2 >= sx^2 (sum w - q_c)^2 / D is tight, so that a window that
is a few per cent too narrow loses rows.  Plain data and seeded numpy builders; nothing here loads
the engine.  tests/test_prune_plan.py holds every claim made here on the CPU, against the numpy
model of the rule (tests/helpers/prune_ref.py).

Stations.  The bound is an equality when x - c lies along the all-ones direction.  A station is a
gray level P (a row with every component at ordinal P) with three groups of G code vectors:
  ring   G vectors at the station's own projection, displaced perpendicular to the ones direction:
         ring 0, a byte vector (P +- delta alternating), by rho, the others by 1.25 rho .. 1.5 rho (a
         runner-up within a fraction of a per cent gets the row flagged, and the recheck, whose
         sweep has a window of its own, would then repair what the search's window lost);
  lo     one vector on the axis at P - a, D a^2 = ratio rho^2, and G - 1 fillers at the same
         projection 1.5 rho off the axis;
  hi     the same at P + a', D a'^2 = 1.004 ratio rho^2 (a' = a, or a (1 + 2.5e-13), on a tie station).
ratio < 1: the lo axis vector is a gray row's answer, in a tile the row's chunk reaches only
through the bound of the ring tile (rho^2), which is barely enough; ratio > 1: ring 0 wins.
G is a multiple of 32 (of 128 in the wide search, whose window moves in slices of 4 tiles), and the
groups' projections are at least two of prune_order's buckets apart, so every tile (slice) is pure
whatever the arrival order inside a bucket.  Code vectors left over form a lone ring group at a
level of its own above the last station; where the levels have no room for one (D = 12 with ten
stations) they join the lo group of station 0 as fillers in whole multiples of G and the last
station's hi group with the remainder.  Either way the remainder has the highest projection, so
that the last tile is partly padding.

Every codebook lies in [vmin, vmax] (a legal C_start of qvq_refine); rows are oracle.lut(cs)[codes].
Field values as in largek_cases.py: search mf32 | wide, recheck mf32 | staged | chunked | global."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from helpers import prune_ref as pr  # noqa: E402

COLOUR = {"scaled": oracle.SCALED, "normal": oracle.NORMAL}
RHO = 30.0            # the ring radius aimed at, in table steps (one step = 2 sx)
TIE_REL = 1e-12       # the reference's tie band (relative)


def _values(U, cs):
    """Real-valued ordinals -> values."""
    mu, sx = pr.TERMS[cs]
    return mu + (2.0 * np.asarray(U, np.float64) - 255.0) * sx


def _delta(D):
    n = D - D % 2
    return max(1, int(round(RHO / np.sqrt(n))))


def _pattern(D):
    """The +-1 alternating direction over the first D - D % 2 components (sum 0)."""
    s = np.zeros(D)
    n = D - D % 2
    s[:n:2], s[1:n:2] = 1.0, -1.0
    return s


def _perp(rng, D):
    """A random unit vector perpendicular to the ones direction: balanced random signs from D = 8
    (components 1 / sqrt(n): the vectors stay inside the value range), a Gaussian one below."""
    if D >= 8:
        n = D - D % 2
        s = np.zeros(D)
        s[rng.permutation(D)[:n]] = rng.permutation(np.repeat([1.0, -1.0], n // 2))
        return s / np.sqrt(n)
    v = rng.normal(size=D)
    v -= v.mean()
    return v / np.sqrt(v @ v)


def station_codebook(D, K, G, ratios, ties, seed):
    """(U [K, D] real ordinals in index order, stations): the stations' levels, and per station the
    indices of ring 0, the lo axis and the hi axis vector, and its ratio / tie kind."""
    rng = np.random.default_rng(seed)
    S = len(ratios)
    delta = _delta(D)
    n = D - D % 2
    rho = delta * np.sqrt(n)
    a = [rho * np.sqrt(r / D) for r in ratios]
    reach = 1.5 * rho * (1 / np.sqrt(n) if D >= 8 else np.sqrt(2.0 / 3.0) if D == 3 else 1.0) + max(a) * 1.01 + 1
    lo_level, hi_level = int(np.ceil(reach)), int(np.floor(255 - reach))
    spare = K - 3 * G * S
    assert spare >= 0
    # the code vectors left over: a lone group of their own above the last station where the
    # levels have room for one, fillers of existing groups where they have not
    half = [x * 1.01 for x in a]
    lone = spare > 0 and sum(h0 + h1 + 3 for h0, h1 in zip(half + [0.0], (half + [0.0])[1:])) <= hi_level - lo_level
    if lone:
        half.append(0.0)
    gaps = [h0 + h1 + 3 for h0, h1 in zip(half, half[1:])]
    span = sum(gaps)
    assert span <= hi_level - lo_level, "stations do not fit: span %.1f of %d" % (span, hi_level - lo_level)
    slack = (hi_level - lo_level - span) / max(1, len(half) - 1)   # spread evenly; integer levels
    P = [lo_level]
    for g in gaps:
        P.append(P[-1] + int(np.floor(g + slack)))
    assert P[-1] <= hi_level
    rows, st = [], []
    for s in range(S):
        ring = [P[s] + delta * _pattern(D)] + [P[s] + rho * (1.25 + 0.25 * j / G) * _perp(rng, D) for j in range(1, G)]
        a_hi = a[s] * np.sqrt(1.004)
        if ties[s] == "exact":
            a_hi = a[s]
        elif ties[s] == "close":
            a_hi = a[s] * (1 + 2.5e-13)
        n_lo = G + (spare // G * G if s == 0 and not lone else 0)
        n_hi = G + (spare % G if s == S - 1 and not lone else 0)
        lo = [np.full(D, P[s] - a[s])] + [P[s] - a[s] + 1.5 * rho * _perp(rng, D) for _ in range(n_lo - 1)]
        hi = [np.full(D, P[s] + a_hi)] + [P[s] + a_hi + 1.5 * rho * _perp(rng, D) for _ in range(n_hi - 1)]
        base = len(rows)
        st.append({"P": P[s], "ratio": ratios[s], "tie": ties[s], "ring0": base, "lo": base + G,
                   "hi": base + G + n_lo, "first": base, "count": G + n_lo + n_hi})
        rows += ring + lo + hi
    if lone:
        rows += [P[S] + rho * (1.25 + 0.25 * j / spare) * _perp(rng, D) for j in range(spare)]
    U = np.array(rows)
    assert U.shape == (K, D)
    order = rng.permutation(K)          # index order: anything but the projection order
    inv = np.empty(K, np.int64)
    inv[order] = np.arange(K)
    for s in st:
        s["members"] = inv[s["first"]:s["first"] + s["count"]]
        for f in ("ring0", "lo", "hi"):
            s[f] = int(inv[s[f]])
    return U[inv.argsort()], st, delta


# row patterns: which rows of a window group are gray ("far": their answer is an axis vector when
# the station's ratio < 1) and which sit on ring 0 (best distance 0)
def _far_mask(pattern, chunks):
    """bool per row of the group's chunks (concatenated)."""
    out = []
    for ci, rows in enumerate(chunks):
        r = rows % pr.CHUNK
        if pattern == "all":
            m = np.ones(len(rows), bool)
        elif pattern == "alt":
            m = r % 2 == 0
        elif pattern == "row0":
            m = r == 0
        elif pattern == "row63":
            m = r == 63
        elif pattern == "rows32_63":
            m = r >= 32
        elif pattern == "wave_first":
            m = np.full(len(rows), ci == 0)
        elif pattern == "wave_last":
            m = np.full(len(rows), ci == len(chunks) - 1)
        else:
            raise ValueError(pattern)
        out.append(m)
    return np.concatenate(out)


def build_stations(c):
    """(rows X, codebook C, info) of a station case.  info: station of every row (-1: an end row),
    far (bool per row: a gray row), the stations."""
    cs = COLOUR[c["cs"]]
    D, K, N = c["D"], c["K"], c["N"]
    U, st, delta = station_codebook(D, K, c["G"], c["ratios"], c["ties"], c["seed"])
    S = len(st)
    grp = pr.groups(N, c["kind"], c.get("cpr", 1))
    station = np.zeros(N, np.int64)
    far = np.ones(N, bool)
    ring0 = delta * _pattern(D)
    codes = np.zeros((N, D), np.int64)
    for g, chunks in enumerate(grp):
        rows = np.concatenate(chunks)
        s = g % S
        station[rows] = s
        if c["pattern"] == "two":       # a chunk holding two far-apart stations
            other = (s + S // 2) % S
            station[rows[rows % pr.CHUNK >= 32]] = other
        else:
            far[rows] = _far_mask(c["pattern"], chunks)
    # a ragged last chunk holds far rows whatever the pattern
    if N % pr.CHUNK:
        far[N - N % pr.CHUNK:] = True
    level = np.array([s["P"] for s in st])[station]
    codes[:] = level[:, None]
    codes[~far] += ring0.astype(np.int64)
    if c.get("ends"):                   # rows below every envelope, rows above every envelope
        tail = np.concatenate(grp[-2]), np.concatenate(grp[-1])
        for rows, lv in zip(tail, (1, 254)):
            codes[rows] = lv
            station[rows] = -1
            far[rows] = True
    assert codes.min() >= 0 and codes.max() <= 255
    lut = oracle.lut(cs)
    X = np.ascontiguousarray(lut[(codes ^ 0x80).astype(np.uint8)])
    C = np.ascontiguousarray(_values(U, cs))
    return X, C, {"station": station, "far": far, "stations": st, "codes": (codes ^ 0x80).astype(np.uint8)}


def build_degenerate(c):
    """(rows, codebook, info): orders that give prune_order nothing, or little, to sort by."""
    cs = COLOUR[c["cs"]]
    D, K, N = c["D"], c["K"], c["N"]
    rng = np.random.default_rng(c["seed"])
    what = c["degenerate"]

    def perms(levels, n):
        return np.array([rng.permutation(levels) for _ in range(n)], np.float64)
    if what == "one":          # every code vector a permutation of one multiset: one projection
        U = perms(rng.integers(20, 236, D), K)
        codes = rng.integers(0, 256, (N, D))
    elif what == "two":        # two clusters
        U = np.concatenate([perms(rng.integers(10, 90, D), K // 2), perms(rng.integers(160, 250, D), K - K // 2)])
        codes = np.concatenate([rng.integers(0, 100, (N // 2, D)), rng.integers(150, 256, (N - N // 2, D))])
    elif what == "outlier":    # one outlier squeezes every other code vector into a few buckets
        U = np.concatenate([np.full((1, D), 255.0), rng.uniform(2.0, 12.0, (K - 1, D))])
        codes = rng.integers(0, 16, (N, D))
        codes[::97] = 255 - rng.integers(0, 3, (len(codes[::97]), D))
    elif what == "dups":       # duplicates of one code vector fill whole tiles
        base = rng.uniform(0.0, 255.0, (K - 96, D))
        U = np.concatenate([base, np.repeat(base[:1], 96, axis=0)])
        codes = rng.integers(0, 256, (N, D))
        codes[::5] = np.clip(np.rint(base[0]) + rng.integers(-3, 4, (len(codes[::5]), D)), 0, 255)
    else:
        raise ValueError(what)
    U = U[rng.permutation(K)]
    lut = oracle.lut(cs)
    codes = (codes.astype(np.int64) ^ 0x80).astype(np.uint8)
    return np.ascontiguousarray(lut[codes]), np.ascontiguousarray(_values(U, cs)), {"codes": codes}


# ---------------------------------------------------------------------------------------------
# The table.  plan: the qvq_plan fields the case is there for;  first: K - 1 is not pruned (the
# first pruned K of that width);  mutations: the prune_ref.Mutation each of which loses >= 64 rows
# in the model;  prunes: the documented rule visits <= half of the tiles;  geometry: (xs, ys) of
# the raster the rows are laid out as (4 x 4 blocks, qvq_set_images), None: qvq_set_vectors.
# ---------------------------------------------------------------------------------------------
M = pr.Mutation
HALF, QUARTER = M(factor=0.5), M(factor=0.25)
MIN, FIRST, ROWS32 = M(reduce="min"), M(reduce="first"), M(rows32=True)
QHALF, DHALF, PAD = M(q_half=True), M(d_half=True), M(pad=True)
MUT_NAMES = {HALF: "bound x 1/2", QUARTER: "bound x 1/4", M(factor=0.9): "bound x 0.9", M(factor=0.95): "bound x 0.95",
             MIN: "minimum for maximum", FIRST: "first chunk's maximum", ROWS32: "rows 0-31 only",
             QHALF: "q in units of 2w", DHALF: "D / 2", PAD: "pad bytes in sum w"}
_MF = {"search": "mf32", "prune": 1}
_WIDE = {"search": "wide", "cb_resident": 0, "prune": 1}
FAR4, MIXR = [0.9, 0.99, 0.9, 0.99], [0.9, 0.99, 1.01, 1.1]


def _ratios(S, kinds):
    return [kinds[i % len(kinds)] for i in range(S)]


def _s(name, D, K, S, G, kind, plan, ratios=None, ties=None, pattern="all", N=4096, muts=(), prunes=True,
       first=False, cpr=1, geometry=None, ends=False, both=True, recheck=False):
    ratios = _ratios(S, ratios or MIXR)
    return {"name": name, "family": "stations", "D": D, "K": K, "G": G, "kind": kind, "plan": plan, "ratios": ratios,
            "ties": _ratios(S, ties or [None]), "pattern": pattern, "N": N, "mutations": list(muts), "prunes": prunes,
            "first": first, "cpr": cpr, "geometry": geometry, "ends": ends, "both": both, "recheck": recheck}


def _d(name, D, K, kind, plan, what, N=2048):
    return {"name": name, "family": "degenerate", "D": D, "K": K, "kind": kind, "plan": plan, "degenerate": what,
            "N": N, "mutations": [], "prunes": False, "first": False, "cpr": 1, "geometry": None, "both": False,
            "recheck": False, "ties": [None], "pattern": None}


_T = ["exact", "close"]
_T3 = ["exact", "close", None]
TABLE = [
    # ---- stations, D = 12 (assign_mf32_kernel PRUNE: one window per 64-row chunk)
    _s("stations", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1, recheck="mf32"),
       muts=[HALF, QUARTER, M(factor=0.9), M(factor=0.95), QHALF, DHALF]),
    _s("far", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1, recheck="mf32"), ratios=FAR4, muts=[HALF, QUARTER, M(factor=0.9)]),
    _s("ties", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1, recheck="mf32"), ratios=[0.9, 0.99], ties=_T3,
       muts=[HALF, QUARTER]),
    # ---- mixed chunks: the far rows are a minority, the others have best distance 0
    _s("mixed-alt", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=[0.9], pattern="alt", muts=[HALF, MIN]),
    _s("mixed-row0", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=[0.9], pattern="row0", muts=[HALF, MIN]),
    _s("mixed-row63", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=[0.9], pattern="row63",
       muts=[HALF, MIN, ROWS32]),
    _s("mixed-rows32-63", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=[0.9], pattern="rows32_63",
       muts=[HALF, MIN, ROWS32]),
    # ---- range and ends
    _s("two-stations", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=FAR4, pattern="two", prunes=False),
    _s("ends", 12, 1024, 10, 32, "mf32", dict(_MF, fused=1), ratios=FAR4, ends=True, muts=[HALF]),
    _s("ragged", 12, 1000, 10, 32, "mf32", dict(_MF, fused=1), ratios=[0.9], pattern="alt", N=4096 + 37, muts=[HALF, MIN]),
    # ---- K edges, D = 12
    _s("first", 12, 256, 2, 32, "mf32", dict(_MF, fused=1, recheck="staged"), ratios=[0.9, 0.99], first=True,
       muts=[HALF, QUARTER]),
    _s("lanes", 12, 2048, 10, 64, "mf32", dict(_MF, fused=0, c32_staged=0, recheck="staged"), ratios=FAR4,
       muts=[HALF, QUARTER]),
    _s("odd", 12, 2030, 10, 64, "mf32", dict(_MF, fused=0, c32_staged=0, recheck="staged"), ratios=FAR4, ties=_T,
       muts=[HALF, QUARTER]),
    # ---- the wide search, D = 48 (assign_wide_kernel PRUNE: one window per workgroup of 8 chunks)
    _s("first", 48, 1024, 2, 128, "wide", dict(_WIDE, recheck="chunked"), ratios=[0.9, 0.99], first=True,
       muts=[HALF, QUARTER, DHALF]),
    _s("scan2", 48, 2100, 5, 128, "wide", dict(_WIDE, recheck="chunked"), ratios=FAR4, muts=[HALF, QUARTER]),
    _s("odd", 48, 4000, 10, 128, "wide", dict(_WIDE, recheck="chunked"), ratios=FAR4, muts=[HALF, M(factor=0.9), QHALF]),
    _s("full", 48, 4096, 10, 128, "wide", dict(_WIDE, recheck="chunked"), ratios=MIXR, muts=[HALF], both=False),
    _s("wave-first", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="wave_first", muts=[HALF, MIN]),
    _s("wave-last", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="wave_last", muts=[HALF, MIN, FIRST]),
    _s("ragged", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="alt", N=4096 + 64 + 37, muts=[HALF, MIN]),
    # the recheck's pruned sweep: ties at a (D, K) whose flagged rows go through recheck_chunked_kernel
    _s("recheck", 48, 1200, 3, 128, "wide", dict(_WIDE, recheck="chunked"), ratios=[0.9, 0.99], ties=_T,
       muts=[HALF, QUARTER], recheck=True),
    # image geometry: the same kind of rows as 4 x 4 blocks of a raster, cpr = 1, 2 and 3
    _s("cpr1", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="wave_last", N=72 * 64, cpr=1,
       geometry=(288, 256), muts=[HALF, FIRST], both=False),
    _s("cpr2", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="wave_last", N=36 * 128, cpr=2,
       geometry=(144, 512), muts=[HALF, FIRST], both=False),
    _s("cpr3", 48, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9], pattern="wave_last", N=27 * 192, cpr=3,
       geometry=(108, 768), muts=[HALF, FIRST], both=False),
    # ---- D = 3 and the pad widths at their first pruned K
    _s("first", 3, None, 4, 128, "wide", dict(_WIDE), ratios=[0.9, 0.99], first=True, muts=[HALF], both=False),
    _s("first", 13, None, 2, 128, "wide", dict(_WIDE), ratios=[0.9, 0.99], ties=_T, first=True, muts=[HALF, PAD]),
    _s("first", 27, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9, 0.99], ties=_T, first=True, muts=[HALF, PAD]),
    _s("first", 46, 1024, 2, 128, "wide", dict(_WIDE), ratios=[0.9, 0.99], ties=_T, first=True, muts=[HALF, PAD]),
    # ---- degenerate orders
    _d("one-projection", 12, 512, "mf32", dict(_MF, fused=1), "one"),
    _d("two-clusters", 12, 512, "mf32", dict(_MF, fused=1), "two"),
    _d("outlier", 12, 512, "mf32", dict(_MF, fused=1), "outlier"),
    _d("duplicates", 12, 512, "mf32", dict(_MF, fused=1), "dups"),
    _d("one-projection", 48, 1024, "wide", dict(_WIDE), "one"),
    _d("outlier", 48, 1024, "wide", dict(_WIDE), "outlier"),
]
# the first pruned K of the widths whose table row leaves K to the engine's capacity rule
# (a codebook resident in LDS is searched unpruned): recorded, and checked by test_prune_plan.py
FIRST_K = {3: 2049, 13: 1121}
# cases whose first seed made the reference's tie rule answer every tie row from the same side
# (a "close" station always answers lo, the nearer one; an exact one is a coin that the tree's
# shape tosses, and these cases have one of each): key(case) -> the first later seed that gives both
RESEED = {"D13-K1121-first-normal": 1, "D27-K1024-first-scaled": 26, "D27-K1024-first-normal": 1}
# the mutations that the scaled case alone is declared for (NORMAL's pad byte has w = 1)
SCALED_ONLY = {PAD}


def key(c):
    return "D%d-K%d-%s-%s" % (c["D"], c["K"], c["name"], c["cs"])


def _cases():
    out = []
    for i, row in enumerate(TABLE):
        for cs in ("scaled", "normal") if row["both"] else ("scaled",):
            c = dict(row, cs=cs)
            if c["K"] is None:
                c["K"] = FIRST_K[c["D"]]
            c["seed"] = 7000 + 10 * i + (1 if cs == "normal" else 0) + 100000 * RESEED.get(key(c), 0)
            c["mutations"] = [m for m in row["mutations"] if cs == "scaled" or m not in SCALED_ONLY]
            c["has_ties"] = any(t is not None for t in c["ties"])
            out.append(c)
    assert len({key(c) for c in out}) == len(out)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _inputs(k):
    c = next(c for c in CASES if key(c) == k)
    X, C, info = (build_stations if c["family"] == "stations" else build_degenerate)(c)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C, info


def inputs(c):
    """(rows, codebook, info) of a case, built once per process; rows and codebook read-only."""
    return _inputs(key(c))


def raster(c):
    """The case's rows as the bytes of an xs x ys raster of 4 x 4 blocks (rows run down the
    image's columns of blocks, as the reference tiles)."""
    xs, ys = c["geometry"]
    return oracle.untile(inputs(c)[2]["codes"], xs, ys, 4, 4)


# ---------------------------------------------------------------------------------------------
# qvq_lbg's own levels.  They take no caller codebook, and they search split codebooks (every
# centroid times 1.2 and times 0.8, so up to 1.2 vmax) that qvq_refine cannot be given.  The split
# moves a gray cell's two children along the all-ones direction, 20 % of the gray level away from
# the cell's rows: the bound is tight for them once the code vectors at the rows' own projection
# are coloured, between one and two times as far off the axis.  Rows run down the image's columns
# of blocks; the first columns are gray, in runs of one level, the others coloured:
#   "patterns"  blocks m +- delta over npat random balanced sign patterns, at the means m = x / 1.2
#               of the gray levels x (their brighter children land on the gray rows' projection);
#   "ray"       blocks m (1 + kappa s0 + noise n_h), m uniform over mrange, s0 the alternating
#               pattern and n_h one of nhue random ones: one coloured ray from the origin, which the
#               split moves along itself, with cells alive at every level.
# Several constructions and seeds were measured with the model on oracle.lbg's split codebooks
# (DESIGN.md 6.6); these are the sharpest.  lost_quarter: rows lost in the model at the pruned
# levels under a quarter of the bound, pinned by tests/test_prune_plan.py (on the gray rows for
# the wide image: its workgroups there are whole gray runs).
# ---------------------------------------------------------------------------------------------
LBG_IMAGES = [
    {"name": "patterns-2x2", "S": 256, "block": 2, "bits": 10, "kind": "mf32", "cpr": 1, "levels": [8, 9, 10],
     "how": "patterns", "grays": [96, 144, 192], "gray_cols": 12, "delta": 28, "npat": 64, "seed": 3,
     "model_rows": None, "lost_quarter": [434, 744, 1984]},
    {"name": "ray-4x4", "S": 512, "block": 4, "bits": 12, "kind": "wide", "cpr": 2, "levels": [10, 11, 12],
     "how": "ray", "grays": [100, 150], "gray_cols": 8, "kappa": 0.3, "noise": 0.08, "nhue": 32, "mrange": (30, 180),
     "seed": 2, "model_rows": 2048, "lost_quarter": [1024, 1024, 1024]},
]


@functools.lru_cache(maxsize=None)
def _lbg_raster(name):
    im = next(i for i in LBG_IMAGES if i["name"] == name)
    rng = np.random.default_rng(im["seed"])
    b, S = im["block"], im["S"]
    D, nb = 3 * b * b, S // b
    blocks = np.zeros((nb * nb, D), np.int64)     # row = column of blocks * nb + block in the column
    col = 0
    if im["how"] == "patterns":
        pats = np.array([rng.permutation(np.repeat([1, -1], D // 2)) for _ in range(im["npat"])])
        for x in im["grays"]:
            blocks[col * nb:(col + im["gray_cols"]) * nb] = x
            col += im["gray_cols"]
        k = 0
        for c in range(col, nb):
            m = int(round(im["grays"][(c - col) % len(im["grays"])] / 1.2))
            for j in range(nb):
                blocks[c * nb + j] = m + im["delta"] * pats[k % im["npat"]]
                k += 1
    else:
        s0 = np.tile([1.0, -1.0], D // 2)
        hues = np.array([rng.permutation(np.repeat([1.0, -1.0], D // 2)) for _ in range(im["nhue"])])
        for x in im["grays"]:
            blocks[col * nb:(col + im["gray_cols"]) * nb] = x
            col += im["gray_cols"]
        n = (nb - col) * nb
        m = rng.integers(im["mrange"][0], im["mrange"][1] + 1, n)
        h = rng.integers(0, im["nhue"], n)
        blocks[col * nb:] = np.rint(m[:, None] * (1 + im["kappa"] * s0[None, :] + im["noise"] * hues[h]))
    assert blocks.min() >= 0 and blocks.max() <= 255
    rgb = oracle.untile((blocks ^ 0x80).astype(np.uint8), S, S, b, b)
    rgb.setflags(write=False)
    return rgb


def lbg_raster(image):
    """The image's raster bytes (S x S x 3), built once per process and read-only."""
    return _lbg_raster(image["name"])
