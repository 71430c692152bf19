"""The k-means++ case table: each case is a set of row ordinals o [N, dim], a colour space, K, a seed
and the claim it exists for.  tests/test_kmeanspp_cpu.py measures every claim on the restatement
(tests/helpers/kmeanspp_ref.py) and holds the sizes to qvq_host_kmeanspp_plan;
tests/test_gpu_kmeanspp.py runs the cases on the device.  The sizes of the segment, block and cap
cases come from quant_amd.host_kmeanspp_plan, so they follow the launch shape."""
import functools

import numpy as np

import quant_amd
from helpers import kmeanspp_ref as ref

NORMAL, SCALED = ref.NORMAL, ref.SCALED
SEED_SEARCH = 4000   # seeds tried by a case that looks for one
# The cases' names, fixed here so that a test module can be collected without building the table:
# the table takes its sizes from libqvq.so, which a GPU process must not load before torch's
# runtime.  test_kmeanspp_cpu.py holds the tuple to the table.
NAMES = ("one_row", "two_rows", "all_equal", "three_rows", "more_seeds_than_rows", "boundary_0", "boundary_1",
         "boundary_2", "past_32_bits", "rows_block_minus", "rows_block", "rows_block_plus", "rows_segs_minus",
         "rows_segs_plus", "rows_cap_plus", "rows_select_wide", "k4096", "k300", "k300_d48", "dim1", "dim3", "dim5",
         "dim12", "dim13", "dim48", "dim63", "dim64", "pad_valued_scaled", "pad_valued_normal")


def _rng(seed):
    return np.random.default_rng(seed)


def _uniform(n, dim, seed, lo=0, hi=256):
    return _rng(seed).integers(lo, hi, (n, dim))


@functools.lru_cache(maxsize=None)
def plan(n=1):
    return quant_amd.host_kmeanspp_plan(n)


def block():
    return plan()["block"]


def cap():
    return plan()["segments_cap"]


def _three_rows():
    """1000 rows of dim 12 taking three values: ordinals 0, 1 or 2 on every component."""
    return np.repeat(_rng(8).integers(0, 3, 1000)[:, None], 12, axis=1)


def _pad_valued(dim, cs):
    """Real components that take the pad's ordinal (SCALED 0, NORMAL 128) among others: a pad byte
    read with another ordinal than a real byte of the same code shows as a wrong weight."""
    pad = 0 if cs == SCALED else 128
    u = _uniform(700, dim, 90 + dim, 0, 256)
    u[_rng(3).random((700, dim)) < 0.4] = pad
    return u


def _boundary():
    return _uniform(64, 1, 12, 0, 4)


def _two_values():
    """Every row all-0 or all-255 over 64 components: potential[0] is past 2^32."""
    return np.repeat(_rng(21).integers(0, 2, 8257)[:, None] * 255, 64, axis=1)


def _edge_rows(n, dim=3):
    """Rows near each other but for the last row of every segment and the first of the next,
    which lie far out: draws land on them."""
    u = _uniform(n, dim, 400 + n % 97, 120, 136)
    sr = plan(n)["seg_rows"]
    for k in range(1, plan(n)["segments"]):
        u[k * sr - 1] = _rng(k).integers(0, 16, dim)
        u[k * sr] = _rng(k + 50).integers(240, 256, dim)
    return u


def _wanted_edges(n):
    sr, segs = plan(n)["seg_rows"], plan(n)["segments"]
    return {k * sr - 1 for k in range(1, segs)}, {k * sr for k in range(1, segs)}


def _edge_seed(n, K):
    """The first seed whose draws take the last row of a segment and the first row of the next."""
    u = _edge_rows(n)
    last, first = _wanted_edges(n)
    for seed in range(SEED_SEARCH):
        rows = set(int(r) for r in ref.kmeanspp(u, K, seed)[0][1:])
        if rows & last and rows & first:
            return seed
    raise AssertionError("no seed draws both sides of a segment edge")


def _boundary_seeds(count=3):
    """Seeds whose draws on the boundary set hit t == prefix[s - 1] behind a row with m = 0."""
    u, out = _boundary(), []
    for seed in range(SEED_SEARCH):
        tr = ref.kmeanspp(u, 4, seed)[3]
        if sum(d["boundary"] and d["zero_before"] for d in tr) >= 2:
            out.append(seed)
            if len(out) == count:
                return out
    raise AssertionError("too few boundary seeds")


def _case(claim, build, cs, K, seed=0):
    return {"claim": claim, "build": build, "cs": cs, "K": K, "seed": seed}


def _table():
    B, S = block(), cap()
    two_seg = 2 * plan(2 * B + 1)["seg_rows"]   # k * seg_rows with k = 2 where seg_rows is one block
    big = S * B + 1                             # the first N whose seg_rows exceeds one block
    wide = S * 1024 + 1                         # the select's lanes take more than one row each
    t = {
        # degenerate sets
        "one_row": _case("N = 1: one seed, potential 0", lambda: _uniform(1, 1, 1), SCALED, 1),
        "two_rows": _case("K = N = 2: both rows, the second potential 0", lambda: np.array([[3, 9, 200], [4, 9, 100]]), NORMAL, 2),
        "all_equal": _case("all rows equal: placed = 1", lambda: np.tile(_uniform(1, 12, 2), (1024, 1)), SCALED, 5),
        "three_rows": _case("three distinct rows, K = 8: placed = 3, the potentials end in 0", _three_rows, SCALED, 8),
        "more_seeds_than_rows": _case("K > N: placed <= N", lambda: _uniform(5, 3, 4), NORMAL, 9),
        # the strict comparison
        **{"boundary_%d" % i: _case("t lands on a prefix sum behind a row with m = 0", _boundary, SCALED, 4, s)
           for i, s in enumerate(_boundary_seeds())},
        # totals past 32 bits
        "past_32_bits": _case("potential[0] and the first T are past 2^32", _two_values, NORMAL, 3, 1),
        # segment, block and cap edges (sizes from the plan)
        "rows_block_minus": _case("rows just below a block", lambda: _uniform(B - 1, 3, 31), SCALED, 8),
        "rows_block": _case("rows = a block", lambda: _uniform(B, 3, 32), SCALED, 8),
        "rows_block_plus": _case("rows just above a block: a second segment of one row", lambda: _uniform(B + 1, 3, 33), NORMAL, 8),
        "rows_segs_minus": _case("rows = 2 seg_rows - 1, draws on both sides of a segment edge",
                                 lambda: _edge_rows(two_seg - 1), SCALED, 8, _edge_seed(two_seg - 1, 8)),
        "rows_segs_plus": _case("rows = 2 seg_rows + 1, draws on both sides of a segment edge",
                                lambda: _edge_rows(two_seg + 1), NORMAL, 8, _edge_seed(two_seg + 1, 8)),
        "rows_cap_plus": _case("rows = segments_cap * block + 1: seg_rows exceeds one block",
                               lambda: _uniform(big, 3, 36, 0, 64), SCALED, 8, 2),
        "rows_select_wide": _case("seg_rows past the select's lanes: a lane of its row scan takes two rows",
                                  lambda: _uniform(wide, 1, 37, 0, 256), NORMAL, 4, 3),
        # many seeds
        "k4096": _case("4095 dependent rounds", lambda: _uniform(8257, 12, 41), SCALED, 4096, 5),
        "k300": _case("K not a power of two", lambda: _uniform(8257, 12, 42), NORMAL, 300, 6),
        "k300_d48": _case("K not a power of two, D = 48", lambda: _uniform(4097, 48, 43), SCALED, 300, 7),
    }
    # row widths: every pad remainder (pads 3, 1, 3, 0, 3, 0, 1, 0), NORMAL so that a pad left out of
    # one side of a weight shows (its ordinal is 128), and SCALED with real bytes at the pad's ordinal
    for dim in (1, 3, 5, 12, 13, 48, 63, 64):
        t["dim%d" % dim] = _case("row width %d" % dim, functools.partial(_uniform, 900, dim, 10 + dim), NORMAL, 16, dim)
    t["pad_valued_scaled"] = _case("real bytes at the pad's ordinal (0)", lambda: _pad_valued(5, SCALED), SCALED, 16, 1)
    t["pad_valued_normal"] = _case("real bytes at the pad's ordinal (128)", lambda: _pad_valued(13, NORMAL), NORMAL, 16, 2)
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
    """The restatement's (rows, potential, placed, trace) for the case: computed once, shared."""
    c = table()[name]
    out = ref.kmeanspp(rows(name), c["K"], c["seed"])
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's (C, rows, potential, placed) for the case."""
    r, pot, placed, _ = trace(name)
    C = ref.codebook(rows(name), table()[name]["cs"], r, placed)
    C.setflags(write=False)
    return C, r, pot, placed
