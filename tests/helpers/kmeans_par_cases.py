"""The k-means|| case table: each case is a set of row ordinals o [N, dim], a colour space, K, a seed,
the options and the claim it exists for.  tests/test_kmeans_par_cpu.py measures every claim on the
restatement (tests/helpers/kmeans_par_ref.py) and holds the sizes to qvq_host_kmeans_par_plan;
tests/test_gpu_kmeans_par.py runs the cases on the device.  The sizes of the block, segment, cap,
chunk and LDS cases come from quant_amd.host_kmeans_par_plan, so they follow the launch shape."""
import functools

import numpy as np

import quant_amd
from helpers import kmeans_par_ref as ref

NORMAL, SCALED = ref.NORMAL, ref.SCALED
SEED_SEARCH = 20000   # seeds tried by a case that looks for one
WIDTHS = (1, 2, 3, 4, 5, 12, 13, 48, 61, 64)
# The cases' names, fixed here so that a test module can be collected without building the table:
# the table takes its sizes from libqvq.so, which a GPU process must not load before torch's
# runtime.  test_kmeans_par_cpu.py holds the tuple to the table.
NAMES = ("one_row", "all_equal", "few_distinct", "k_gt_m", "rows_block_minus", "rows_block", "rows_block_plus",
         "rows_segs_minus", "rows_segs", "rows_segs_plus", "rows_cap_minus", "rows_cap", "rows_cap_plus", "truncate",
         "same_round_twins", "near_tie", "join_boundary", "phi_past_32_bits", "reduction_past_32_bits", "chunk_minus",
         "chunk_exact", "chunk_plus", "lds_in", "lds_out", "gw_global", "k1", "k37", "k300", "rounds1", "rounds16",
         "pad_valued_scaled", "pad_valued_normal") + tuple("dim%d" % d for d in WIDTHS)


def _rng(seed):
    return np.random.default_rng(seed)


def _uniform(n, dim, seed, lo=0, hi=256):
    return _rng(seed).integers(lo, hi, (n, dim))


@functools.lru_cache(maxsize=None)
def plan(n=1, dim=1, K=1, rounds=0, ell=0, round_cap=0):
    return quant_amd.host_kmeans_par_plan(n, dim, K, rounds, ell, round_cap)


def block():
    return plan()["block"]


def cap():
    return plan()["segments_cap"]


def chunk():
    return plan()["chunk"]


def _three_values():
    """1000 rows of dim 12 taking three values: ordinals 0, 1 or 2 on every component."""
    return np.repeat(_rng(8).integers(0, 3, 1000)[:, None], 12, axis=1)


def _pad_valued(dim, cs):
    """Real components that take the pad's ordinal (SCALED 0, NORMAL 128) among others: a pad byte
    read with another ordinal than a real byte of the same code shows as a wrong weight."""
    pad = 0 if cs == SCALED else 128
    u = _uniform(700, dim, 90 + dim, 0, 256)
    u[_rng(3).random((700, dim)) < 0.4] = pad
    return u


def _synthetic():
    """The 2x2 blocks of a smooth 128 x 128 image with noise: 4096 rows of dim 12."""
    y, x = np.mgrid[0:128, 0:128]
    img = np.stack([(x * 2) % 256, (y * 2) % 256, (x + y) % 256], axis=2) + _rng(77).integers(0, 24, (128, 128, 3))
    img = np.clip(img, 0, 255)
    return img.reshape(64, 2, 64, 2, 3).transpose(0, 2, 1, 3, 4).reshape(4096, 12)


def _twins():
    """256 distinct rows, each present twice (row i and row i + 256)."""
    u = _uniform(256, 3, 55)
    return np.concatenate([u, u])


# near_tie: rows on a line.  100 rows at ordinal 0 (candidate 0 among them), then P at 100, a band of
# 16 rows at 120, Q at 140.  A seed is looked for at which P and Q join round 1 and no band row does:
# the band then lies 20 from both, below its 120 from candidate 0, and takes P, the lower index.
TIE_BAND = 16


def _tie_rows():
    return np.array([0] * 100 + [100] + [120] * TIE_BAND + [140])[:, None]


def _tie_seed():
    u, N = _tie_rows(), 100 + TIE_BAND + 2
    m = (u[:, 0] ** 2).astype(np.uint64)
    phi = int(m.sum())
    for seed in range(SEED_SEARCH):
        if ref.draw(seed, 0, N) >= 100:
            continue
        j = np.flatnonzero(ref.join_values(seed, 1, N, phi) < np.uint64(4) * m)
        if list(j) == [100, 100 + TIE_BAND + 1]:
            return seed
    raise AssertionError("no seed makes the two ends join alone")


# join_boundary: rows at ordinals 0 and 1 on one component, so that phi is about N / 2 and mulhi lands
# on ell * m - 1 and on ell * m for some row of round 1 at about every third seed.
def _boundary_rows():
    return _uniform(64, 1, 12, 0, 2)


def _boundary_seed():
    """The first seed at which round 1 has a row with mulhi = ell * m - 1 and one with mulhi = ell * m, m > 0."""
    u = _boundary_rows()
    for seed in range(SEED_SEARCH):
        tr = ref.kmeans_par(u, 4, seed, rounds=1, ell=4)["trace"]
        if tr and boundary_hits(tr[0]) == (True, True):
            return seed
    raise AssertionError("no seed puts a row on each side of the strict comparison")   # (found: see the claim)


def boundary_hits(round_trace):
    lhs, rhs = round_trace["lhs"], round_trace["rhs"]
    live = rhs > 0
    return bool(np.any(live & (lhs + np.uint64(1) == rhs))), bool(np.any(live & (lhs == rhs)))


def _two_values():
    """Every row all-0 or all-255 over 64 components: the potentials are past 2^32."""
    return np.repeat(_rng(21).integers(0, 2, 4096)[:, None] * 255, 64, axis=1)


def _two_clusters():
    """1033 rows all-0, 1033 all-255 and 96 low rows over 64 components, shuffled.  1033 * 64 * 255^2 is
    2^32 + 3 965 504: the weight of a whole cluster times its g passes 2^32 by little, so a product
    kept in 32 bits all but vanishes from the prefix."""
    u = np.concatenate([np.zeros((1033, 64), np.int64), np.full((1033, 64), 255), _uniform(96, 64, 23, 0, 100)])
    return u[_rng(24).permutation(len(u))]


def truncated_pick(out, u, seed):
    """The reduction's second seed if every product wt * g were kept in 32 bits (None: T = 0)."""
    M = out["info"]["candidates"]
    cu = u[out["cand_rows"][:M].astype(np.int64)]
    g = ((cu - cu[out["picks"][0]]) ** 2).sum(axis=1)
    prod = (out["cand_weights"][:M].astype(np.int64) * g) & 0xFFFFFFFF
    T = int(prod.sum())
    return int(np.searchsorted(np.cumsum(prod), ref.draw((seed + ref.REDUCE_STREAM) & ref.MASK, 1, T), side="right")) if T else None


def _product_seed():
    """The first seed at which a product passes 2^32 and the truncated products draw another candidate."""
    u = _two_clusters()
    for seed in range(200):
        out = ref.kmeans_par(u, 8, seed)
        if out["max_product"][0] > 1 << 32 and truncated_pick(out, u, seed) != out["picks"][1]:
            return seed
    raise AssertionError("no seed tells the 32-bit products apart")


def _lds_cap(side):
    """rounds = 1: the largest round_cap whose candidates' code words sit in the reduction's LDS at
    64 bytes a row (side 0), and the next (side 1)."""
    c = 1
    while plan(4096, 64, 16, 1, 64, c + 1)["codes_lds"]:
        c += 1
    return c + side


def _case(claim, build, cs, K, seed=0, rounds=0, ell=0, round_cap=0):
    return {"claim": claim, "build": build, "cs": cs, "K": K, "seed": seed,
            "opts": {"rounds": rounds, "ell": ell, "round_cap": round_cap}}


def _table():
    B, S, C = block(), cap(), chunk()
    seg = plan(2 * B + 1)["seg_rows"]
    t = {
        # degenerate sets
        "one_row": _case("N = 1: phi_0 = 0, no round samples, M = 1, placed = 1", lambda: _uniform(1, 1, 1), SCALED, 4),
        "all_equal": _case("all rows equal: phi_0 = 0, no round samples, M = 1, placed = 1",
                           lambda: np.tile(_uniform(1, 12, 2), (1024, 1)), SCALED, 5),
        "few_distinct": _case("three distinct rows, K = 8: placed < K", _three_values, SCALED, 8),
        "k_gt_m": _case("rounds = 1, ell = 1, K = 64: M < K, the reduction stops by T = 0",
                        lambda: _uniform(2000, 3, 4), NORMAL, 64, 1, rounds=1, ell=1),
        # block, segment and cap edges (sizes from the plan)
        "rows_block_minus": _case("rows just below a block", lambda: _uniform(B - 1, 3, 31), SCALED, 4),
        "rows_block": _case("rows = a block", lambda: _uniform(B, 3, 32), SCALED, 4),
        "rows_block_plus": _case("rows just above a block: a second segment of one row", lambda: _uniform(B + 1, 3, 33), NORMAL, 4),
        "rows_segs_minus": _case("rows = 2 seg_rows - 1", lambda: _uniform(2 * seg - 1, 3, 34), SCALED, 4),
        "rows_segs": _case("rows = 2 seg_rows", lambda: _uniform(2 * seg, 3, 35), NORMAL, 4),
        "rows_segs_plus": _case("rows = 2 seg_rows + 1", lambda: _uniform(2 * seg + 1, 3, 36), NORMAL, 4),
        "rows_cap_minus": _case("rows = segments_cap * block - 1", lambda: _uniform(S * B - 1, 3, 37, 0, 64), SCALED, 4),
        "rows_cap": _case("rows = segments_cap * block: every segment one full block", lambda: _uniform(S * B, 3, 38, 0, 64), SCALED, 4, 1),
        "rows_cap_plus": _case("rows = segments_cap * block + 1: seg_rows exceeds one block",
                               lambda: _uniform(S * B + 1, 3, 39, 0, 64), NORMAL, 4, 2),
        # the sample
        "truncate": _case("ell = 64, round_cap = 8: rounds truncate, the kept rows are the 8 lowest joiners",
                          _synthetic, SCALED, 64, 0, ell=64, round_cap=8),
        "same_round_twins": _case("every row twice, ell = N: a candidate of weight 0, never a seed",
                                  _twins, NORMAL, 16, 3, rounds=2, ell=512),
        "near_tie": _case("two candidates of round 1 equidistant from a band of 16 rows: all take the lower index",
                          _tie_rows, SCALED, 4, _tie_seed(), rounds=1, ell=4),
        "join_boundary": _case("round 1 has mulhi = ell m - 1 (joins) and mulhi = ell m (does not) (found by search)",
                               _boundary_rows, SCALED, 4, _boundary_seed(), rounds=1, ell=4),
        # totals past 32 bits
        "phi_past_32_bits": _case("phi is past 2^32 when round 1 samples", _two_values, NORMAL, 4, 1),
        "reduction_past_32_bits": _case("a product wt g and the reduction's T are past 2^32; kept in 32 bits they draw another candidate", _two_clusters, NORMAL, 8, _product_seed()),
        # the update's chunk: candidates of a round at the chunk size - 1, exactly, + 1 (by truncation)
        "chunk_minus": _case("rounds of chunk - 1 candidates", lambda: _uniform(2048, 12, 61), SCALED, 16, 1,
                             rounds=2, ell=1024, round_cap=C - 1),
        "chunk_exact": _case("rounds of chunk candidates", lambda: _uniform(2048, 12, 62), SCALED, 16, 2,
                             rounds=2, ell=1024, round_cap=C),
        "chunk_plus": _case("rounds of chunk + 1 candidates: a second trip of one", lambda: _uniform(2048, 12, 63), NORMAL, 16, 3,
                            rounds=2, ell=1024, round_cap=C + 1),
        # the reduction's LDS: decided from max_candidates and the padded width
        "lds_in": _case("the most candidates whose code words sit in the reduction's LDS at 64 bytes a row",
                        lambda: _uniform(4096, 64, 64), SCALED, 16, 4, rounds=1, ell=64, round_cap=_lds_cap(0)),
        "lds_out": _case("one candidate more: the code words are read from global memory",
                         lambda: _uniform(4096, 64, 64), SCALED, 16, 4, rounds=1, ell=64, round_cap=_lds_cap(1)),
        "gw_global": _case("max_candidates past the LDS that holds g and wt: both in global memory",
                           lambda: _uniform(2000, 5, 65), NORMAL, 16, 5, rounds=16, ell=16, round_cap=1300),
        # seeds
        "k1": _case("K = 1: the first draw alone", lambda: _uniform(3000, 3, 41), SCALED, 1, 5),
        "k37": _case("K not a power of two", lambda: _uniform(8257, 12, 42), NORMAL, 37, 6),
        "k300": _case("K = 300, ell = 300: rounds of several chunks", lambda: _uniform(8257, 12, 43), SCALED, 300, 7),
        "rounds1": _case("rounds = 1", lambda: _uniform(3000, 3, 44), SCALED, 16, 8, rounds=1),
        "rounds16": _case("rounds = 16", lambda: _uniform(3000, 3, 45), NORMAL, 16, 9, rounds=16, ell=8),
        "pad_valued_scaled": _case("real bytes at the pad's ordinal (0)", lambda: _pad_valued(5, SCALED), SCALED, 16, 1),
        "pad_valued_normal": _case("real bytes at the pad's ordinal (128)", lambda: _pad_valued(13, NORMAL), NORMAL, 16, 2),
    }
    # row widths: every pad remainder, NORMAL so that a pad left out of one side of a weight shows (its ordinal is 128)
    for dim in WIDTHS:
        t["dim%d" % dim] = _case("row width %d" % dim, functools.partial(_uniform, 900, dim, 10 + dim), NORMAL, 16, dim)
    return t


@functools.lru_cache(maxsize=None)
def table():
    return _table()


def names():
    return list(NAMES)


@functools.lru_cache(maxsize=None)
def rows(name):
    u = np.ascontiguousarray(table()[name]["build"](), dtype=np.int64)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def trace(name):
    """The restatement's dict for the case: computed once, shared."""
    c = table()[name]
    out = ref.kmeans_par(rows(name), c["K"], c["seed"], **c["opts"])
    for k in ("rows", "cand_rows", "cand_weights"):
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's (C, rows, cand_rows, cand_weights, info) for the case."""
    out = trace(name)
    C = ref.codebook(rows(name), table()[name]["cs"], out["rows"], out["info"]["placed"])
    C.setflags(write=False)
    return C, out["rows"], out["cand_rows"], out["cand_weights"], out["info"]
