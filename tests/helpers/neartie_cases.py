"""The cases of tests/test_gpu_neartie.py: codebooks of code vector pairs whose distances to a row
differ by 1e-17 ... 1e-3 relative -- the band where the reference's tie rule leaves the fp64 argmin,
where the recheck's summation order decides the index, and where an fp32 bound that is too small
loses a row.  Plain data and the seeded, pure-numpy input builders; nothing here
loads the engine.

Every case names the qvq_plan fields (include/qvq.h, quant_amd.host_plan) it is there for;
tests/test_neartie_plan.py checks them on the CPU, together with the band's coverage, the number of
rows on which the reference's answer is not the fp64 argmin ("ties" below), and the oracle's answers
against the compiled reference's recorded ones (tests/golden/ref_nn_neartie.json).

Field values are written as in largek_cases.py: search small | mf32 | wide | valu, recheck mf32 |
staged | chunked | global."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

RADII = {"near": (0.02, 0.12), "far": (0.3, 0.6)}      # |x - a| in units of vmax - vmin
BASE_ROWS = {"near": 2048, "far": 4096}
DECADES = list(range(-17, -2))                         # 2 delta = mantissa * 10^e, e = -17 ... -3
# the decades [10^e, 10^(e+1)) of the relative gap that every case fills with >= MIN_ROWS rows
BAND = list(range(-16, -3))
MIN_ROWS = 5
COLOUR = {"scaled": oracle.SCALED, "normal": oracle.NORMAL}


def build(D, K, cs, regime, seed, copies=None):
    """(rows X, codebook C) of a case.

    Rows: oracle.lut(cs)[codes], so qvq_set_vectors stays on the byte path.  Half of the BASE_ROWS
    codes are uniform bytes; a quarter are bytes 0-15 and 240-255 (values next to mu: the smallest
    sum |w|); a quarter are bytes 112-143 (values at both ends of the value range: the largest
    sum |w|, where the per-row MFMA bound is largest, and where the pairs below must turn inwards).
    Pairs: for M = K / 2 distinct anchor rows x, a direction v of length r (vmax - vmin) with r from
    RADII[regime], a = x + s v, b = x + s' roll(v, 1) (1 + delta): the same squares in another order,
    so the two distances differ by 2 delta relative and by what fp64 rounding makes of the two sums.
    The signs s and s' are random per component and flipped where the component would leave
    [vmin, vmax]; an anchor with a component that fits under neither sign is dropped for the next
    candidate.  2 delta is a uniform mantissa times 10^e with e cycling through DECADES, so each
    anchor aims at one decade of the gap; one anchor in sixteen gets delta = 0.  C interleaves a, b.
    Every anchor row appears `copies` times among the rows (the further copies at the end; the
    default is default_copies(K)), so that a small codebook, or a narrow one whose pairs crowd each
    other out, still puts MIN_ROWS rows into each decade it reaches."""
    rng = np.random.default_rng(seed)
    lut = oracle.lut(cs)
    vmin, vmax = lut.min(), lut.max()
    M, n0 = K // 2, BASE_ROWS[regime]
    assert K == 2 * M
    edge = np.concatenate([np.arange(0, 16), np.arange(240, 256)])
    codes = np.concatenate([rng.integers(0, 256, (n0 // 2, D)),
                            edge[rng.integers(0, 32, (n0 // 4, D))],
                            rng.integers(112, 144, (n0 - n0 // 2 - n0 // 4, D))]).astype(np.uint8)
    codes = codes[rng.permutation(n0)]
    first = np.unique(codes, axis=0, return_index=True)[1]      # one index per distinct row
    lo, hi = RADII[regime]
    C, anchors = [], []
    for i in rng.permutation(first):
        if len(anchors) == M:
            break
        x = lut[codes[i]]
        m = len(anchors)
        delta = 0.0 if m % 16 == 15 else 0.5 * rng.uniform(1, 10) * 10.0 ** DECADES[(m - m // 16) % len(DECADES)]
        v = rng.normal(size=D)
        v *= rng.uniform(lo, hi) * (vmax - vmin) / np.sqrt(v @ v)

        def inwards(step):
            s = rng.choice([-1.0, 1.0], D)
            return np.where((x + s * step >= vmin) & (x + s * step <= vmax), s, -s) * step
        a, b = x + inwards(v), x + inwards(np.roll(v, 1) * (1 + delta))
        if min(a.min(), b.min()) < vmin or max(a.max(), b.max()) > vmax:
            continue
        C += [a, b]
        anchors.append(i)
    assert len(anchors) == M, "only %d of %d anchors fit" % (len(anchors), M)
    codes = np.concatenate([codes] + [codes[anchors]] * ((copies or default_copies(K)) - 1))
    return np.ascontiguousarray(lut[codes]), np.ascontiguousarray(np.array(C))


def default_copies(K):
    return max(1, -(-240 // K))


def rows_of(K, regime, copies=None):
    return BASE_ROWS[regime] + K // 2 * ((copies or default_copies(K)) - 1)


def top_two(X, C):
    """(d1, d2, i1, i2) per row: the two smallest distances over all K in np.longdouble, and the
    code vectors they belong to."""
    # the eight nearest by the expanded form in fp64 (its error, ~1e-15 |x|^2, cannot push one of the
    # true two behind six others), then those eight in long double
    rough = (X * X).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None] - 2.0 * (X @ C.T)
    cand = np.argpartition(rough, 7, axis=1)[:, :8]
    diff = X[:, None, :].astype(np.longdouble) - C[cand].astype(np.longdouble)
    d = (diff * diff).sum(axis=2)
    o = np.argsort(d, axis=1, kind="stable")[:, :2]
    dd = np.take_along_axis(d, o, axis=1)
    ii = np.take_along_axis(cand, o, axis=1)
    return dd[:, 0], dd[:, 1], ii[:, 0], ii[:, 1]


def rel_gap(X, C):
    """(d2 - d1) / d1 per row in np.longdouble, top two of all K (inf where d1 = 0)."""
    d1, d2, _, _ = top_two(X, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d1 > 0, (d2 - d1) / d1, np.inf)


def band_counts(gap):
    """Rows per decade of BAND."""
    return {e: int(np.sum((gap >= 10.0 ** e) & (gap < 10.0 ** (e + 1)))) for e in BAND}


# ---------------------------------------------------------------------------------------------
# The table.  plan: the default dispatch; valu: further fields under QVQ_SEARCH=valu (K > 32);
# refine: the case also runs through qvq_refine (its codebook lies in [vmin, vmax], a legal C_start);
# far: the far regime is run as well; copies: how often every anchor row appears (build).
# Every row runs in SCALED and in NORMAL: mu, sx, the score scale t and the bounds' magnitudes differ.
# K = 32 is the small scan's case: the band's 13 decades need at least 13 pairs, and K <= 32 is that
# kernel's whole range.
# ---------------------------------------------------------------------------------------------
def _c(D, K, plan, valu, refine=False, far=False, copies=None):
    return {"D": D, "K": K, "plan": plan, "valu": valu, "refine": refine, "far": far, "copies": copies}


_MF = {"search": "mf32"}
_WIDE = {"search": "wide"}
TABLE = [
    # D = 12
    _c(12, 32, {"search": "small", "recheck": "staged"}, None, far=True),                  # e0 / e1
    _c(12, 100, dict(_MF, fused=1, c32_staged=1, recheck="staged"), {"valu_tiles": 1}, far=True, copies=5),
    _c(12, 600, dict(_MF, fused=1, prune=1, recheck="mf32"), {"recheck": "staged"}, refine=True, far=True),
    _c(12, 1024, dict(_MF, fused=1, prune=1, recheck="mf32"), {"valu_tiles": 1}, refine=True, far=True),
    _c(12, 1700, dict(_MF, fused=0, prune=1, c32_staged=0, recheck="staged"), {"valu_tiles": 2}, refine=True,
       far=True),
    _c(12, 3200, {"search": "valu", "valu_tiles": 3, "recheck": "chunked"}, {"valu_tiles": 3}, far=True),
    # D = 48
    _c(48, 100, {"search": "valu", "valu_tiles": 1, "recheck": "staged"}, {"valu_tiles": 1}, far=True),
    _c(48, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"recheck": "staged"}, far=True),
    _c(48, 800, dict(_WIDE, cb_resident=0, recheck="chunked"), {"valu_tiles": 3, "recheck": "chunked"}, far=True),
    _c(48, 1200, dict(_WIDE, cb_resident=0, prune=1, recheck="chunked"), {"valu_tiles": 4}, refine=True, far=True),
    # D = 27: one pad byte
    _c(27, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"recheck": "staged"}, far=True),
    _c(27, 1400, dict(_WIDE, cb_resident=0, prune=1, recheck="global"), {"valu_tiles": 3, "recheck": "global"},
       refine=True, far=True),
    # nanoflann's groups of four: three groups and one leftover, one group and one leftover, no group
    _c(13, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"recheck": "staged"}),
    _c(5, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"recheck": "staged"}, copies=3),
    _c(3, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"recheck": "staged"}, copies=4),
    # Dp = 64: wide_ks = 5, the largest `rounds` of mfma_setup
    _c(64, 300, dict(_WIDE, cb_resident=1, recheck="staged"), {"valu_tiles": 2}, far=True),
]

# rows with oracle.kdtree_nn != the fp64 argmin (oracle.bruteforce): the reference's tie rule at work.
# key(case) -> count, recorded from the generator and asserted by tests/test_neartie_plan.py
TIES = {
    "D12-K32-scaled-near": 0,
    "D12-K32-normal-near": 0,
    "D12-K32-scaled-far": 0,
    "D12-K32-normal-far": 8,
    "D12-K100-scaled-near": 5,
    "D12-K100-normal-near": 5,
    "D12-K100-scaled-far": 5,
    "D12-K100-normal-far": 10,
    "D12-K600-scaled-near": 5,
    "D12-K600-normal-near": 8,
    "D12-K600-scaled-far": 7,
    "D12-K600-normal-far": 6,
    "D12-K1024-scaled-near": 4,
    "D12-K1024-normal-near": 6,
    "D12-K1024-scaled-far": 11,
    "D12-K1024-normal-far": 13,
    "D12-K1700-scaled-near": 5,
    "D12-K1700-normal-near": 24,
    "D12-K1700-scaled-far": 12,
    "D12-K1700-normal-far": 25,
    "D12-K3200-scaled-near": 19,
    "D12-K3200-normal-near": 48,
    "D12-K3200-scaled-far": 32,
    "D12-K3200-normal-far": 36,
    "D48-K100-scaled-near": 0,
    "D48-K100-normal-near": 0,
    "D48-K100-scaled-far": 0,
    "D48-K100-normal-far": 3,
    "D48-K300-scaled-near": 1,
    "D48-K300-normal-near": 2,
    "D48-K300-scaled-far": 0,
    "D48-K300-normal-far": 8,
    "D48-K800-scaled-near": 2,
    "D48-K800-normal-near": 5,
    "D48-K800-scaled-far": 7,
    "D48-K800-normal-far": 7,
    "D48-K1200-scaled-near": 2,
    "D48-K1200-normal-near": 7,
    "D48-K1200-scaled-far": 20,
    "D48-K1200-normal-far": 15,
    "D27-K300-scaled-near": 2,
    "D27-K300-normal-near": 2,
    "D27-K300-scaled-far": 7,
    "D27-K300-normal-far": 2,
    "D27-K1400-scaled-near": 5,
    "D27-K1400-normal-near": 18,
    "D27-K1400-scaled-far": 12,
    "D27-K1400-normal-far": 17,
    "D13-K300-scaled-near": 0,
    "D13-K300-normal-near": 7,
    "D5-K300-scaled-near": 6,
    "D5-K300-normal-near": 9,
    "D3-K300-scaled-near": 4,
    "D3-K300-normal-near": 12,
    "D64-K300-scaled-near": 0,
    "D64-K300-normal-near": 4,
    "D64-K300-scaled-far": 4,
    "D64-K300-normal-far": 1,
}


# cases whose first seed left a decade of the band short of MIN_ROWS (one anchor per decade at
# K = 32, crowded pairs at D = 3): key(case) -> the first later seed that fills it
RESEED = {
    "D12-K32-normal-near": 1,
    "D12-K32-scaled-far": 2,
    "D12-K32-normal-far": 5,
    "D3-K300-normal-near": 2,
}


def key(c):
    return "D%d-K%d-%s-%s" % (c["D"], c["K"], c["cs"], c["regime"])


def _cases():
    out = []
    for row in TABLE:
        for regime in ("near", "far") if row["far"] else ("near",):
            for cs in ("scaled", "normal"):
                c = dict(row, cs=cs, regime=regime, N=rows_of(row["K"], regime, row["copies"]))
                c["seed"] = (1000 * row["D"] + row["K"] + (7 if cs == "normal" else 0) + (13 if regime == "far" else 0) +
                             100000 * RESEED.get(key(c), 0))
                c["ties"] = TIES.get(key(c))
                out.append(c)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _inputs(k):
    c = next(c for c in CASES if key(c) == k)
    X, C = build(c["D"], c["K"], COLOUR[c["cs"]], c["regime"], c["seed"], c["copies"])
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def inputs(c):
    """(rows, codebook) of a case, built once per process and read-only."""
    return _inputs(key(c))
