"""The greedy k-means++ case table: each case is a set of row ordinals o [N, dim], a colour space, K,
a seed, a trial count and the claim it exists for.  tests/test_kmeanspp_greedy_cpu.py measures every
claim on the restatement (tests/helpers/kmeanspp_greedy_ref.py) and holds the sizes to
qvq_host_kmeanspp_plan; tests/test_gpu_kmeanspp_greedy.py runs the cases on the device.  The sizes of
the block, segment and cap cases come from quant_amd.host_kmeanspp_plan, so they follow the launch
shape (the segments are qvq_kmeanspp's)."""
import functools

import numpy as np

import quant_amd
from helpers import kmeanspp_greedy_ref as ref

NORMAL, SCALED = ref.NORMAL, ref.SCALED
SEED_SEARCH = 4000   # seeds tried by a case that looks for one
WIDTH_DIMS = tuple(4 * nw - nw % 4 for nw in range(1, 17))   # a row width for every padded width 4 .. 64
# The cases' names, fixed here so that a test module can be collected without building the table
# (it takes its sizes from libqvq.so, which a GPU process must not load before torch's runtime).
# test_kmeanspp_greedy_cpu.py holds the tuple to the table.
NAMES = ("one_row", "two_rows", "three_rows_n", "stop", "more_seeds_than_rows", "same_row", "mirror_tie", "last_trial",
         "boundary_later_trial", "past_32_bits", "trials_1", "trials_2", "trials_9", "trials_16", "rows_block_minus",
         "rows_block", "rows_block_plus", "rows_segs_minus", "rows_segs_plus", "rows_cap_minus", "rows_cap_plus",
         "rows_select_wide", "k300", "k300_d48") + tuple("width_%d" % d for d in WIDTH_DIMS)


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


def _three_values():
    """1000 rows of dim 12 taking three values: ordinals 0, 1 or 2 on every component."""
    return np.repeat(_rng(8).integers(0, 3, 1000)[:, None], 12, axis=1)


def _few_rows():
    """40 rows of one component over 6 values: two trials of a round often draw the same row."""
    return _uniform(40, 1, 5, 0, 6) * 40


def _mirror():
    """One component, the rows 127 + d and 127 - d once each around one row at 127, in an order that is
    not its own mirror image: with the first seed at 127, m is mirror symmetric, and so are the
    potentials of two mirrored candidates."""
    d = np.array([0, 9, -9, 23, 40, -23, -40, 61, -61, 88, 110, -110, -88])
    return (127 + d)[:, None]


def _boundary():
    return _uniform(64, 1, 12, 0, 4)


def _three_far_values():
    """Every row all-0, all-128 or all-255 over 64 components, 20000 rows: each candidate of round 1
    leaves the third of the rows at another value at least 64 * 127^2 away, a sum past 2^32."""
    return np.repeat(np.array([0, 128, 255])[_rng(21).integers(0, 3, 20000)][:, None], 64, axis=1)


def _pad_valued(dim, cs):
    """Real components that take the pad's ordinal (SCALED 0, NORMAL 128) among others: a pad byte
    read with another ordinal than a real byte of the same code shows as a wrong weight."""
    pad = 0 if cs == SCALED else 128
    u = _uniform(600, dim, 90 + dim, 0, 256)
    u[_rng(3).random((600, dim)) < 0.4] = pad
    return u


def _edge_rows(n, dim=3):
    """Rows near each other but for the last row of every segment and the first of the next,
    which lie far out: draws land on them."""
    u = _uniform(n, dim, 400 + n % 97, 120, 136)
    sr = plan(n)["seg_rows"]
    for k in range(1, plan(n)["segments"]):
        u[k * sr - 1] = _rng(k).integers(0, 16, dim)
        u[k * sr] = _rng(k + 50).integers(240, 256, dim)
    return u


def _search(u, K, L, good, what):
    """The first seed whose trace satisfies good(result)."""
    for seed in range(SEED_SEARCH):
        if good(ref.kmeanspp_greedy(u, K, seed, L)):
            return seed
    raise AssertionError("no seed gives " + what)


def same_row_rounds(r):
    """Rounds (j, lo, hi) in which trials lo < hi drew the same row and lo won."""
    out = []
    for j, rec in enumerate(r["trace"], start=1):
        win = int(r["trial"][j])
        out += [(j, win, l) for l in range(win + 1, r["trials"]) if rec["c"][l] == rec["c"][win]]
    return out


def tie_rounds(r):
    """Rounds (j, lo, hi) in which trials lo < hi drew different rows of equal, smallest P and lo won."""
    out = []
    for j, rec in enumerate(r["trace"], start=1):
        win = int(r["trial"][j])
        out += [(j, win, l) for l in range(win + 1, r["trials"])
                if rec["c"][l] != rec["c"][win] and rec["P"][l] == rec["P"][win]]
    return out


def boundary_rounds(r):
    """(j, l) with l > 0 whose draw equals the prefix sum just before the drawn row, behind a row with m = 0."""
    return [(j, l) for j, rec in enumerate(r["trace"], start=1) for l in range(1, r["trials"])
            if rec["boundary"][l] and rec["zero_before"][l]]


def edge_draws(n, r):
    """Do the rounds' candidates take the last row of a segment and the first of the next?"""
    sr, segs = plan(n)["seg_rows"], plan(n)["segments"]
    drawn = set(int(c) for c in r["trial_rows"][1:r["placed"], :r["trials"]].ravel())
    return bool(drawn & {k * sr - 1 for k in range(1, segs)}) and bool(drawn & {k * sr for k in range(1, segs) if k * sr < n})


def _case(claim, build, cs, K, seed=0, trials=0):
    return {"claim": claim, "build": build, "cs": cs, "K": K, "seed": seed, "trials": trials}


def _table():
    B, S = block(), cap()
    two_seg = 2 * plan(2 * B + 1)["seg_rows"]   # k * seg_rows with k = 2 where seg_rows is one block
    t = {
        # degenerate sets, all sixteen trials
        "one_row": _case("N = 1: one seed, potential 0", lambda: _uniform(1, 1, 1), SCALED, 1, 0, 16),
        "two_rows": _case("K = N = 2, L = 16: every trial draws the other row", lambda: np.array([[3, 9, 200], [4, 9, 100]]),
                          NORMAL, 2, 0, 16),
        "three_rows_n": _case("K = N = 3, L = 16", lambda: np.array([[0, 0], [10, 0], [0, 30]]), SCALED, 3, 1, 16),
        "stop": _case("three distinct rows, K = 8: placed = 3 (T = 0), the potentials end in 0", _three_values, SCALED, 8, 0, 3),
        "more_seeds_than_rows": _case("K > N: placed <= N", lambda: _uniform(5, 3, 4), NORMAL, 9, 0, 0),
        # the winner's rules
        "same_row": _case("two trials of a round draw the same row and the lower l wins", _few_rows, SCALED, 4,
                          _search(_few_rows(), 4, 4, same_row_rounds, "a round with one row drawn twice"), 4),
        "mirror_tie": _case("two different rows tie on P (mirrored rows) and the lower l wins", _mirror, NORMAL, 2,
                            _search(_mirror(), 2, 6, tie_rounds, "a round with a tie of two rows"), 6),
        "last_trial": _case("a round is won by l = L - 1", lambda: _uniform(500, 3, 6), SCALED, 6,
                            _search(_uniform(500, 3, 6), 6, 5, lambda r: 4 in r["trial"][1:].tolist(), "a win of the last trial"),
                            5),
        # the strict comparison, on a later trial's stream
        "boundary_later_trial": _case("t_l lands on a prefix sum behind a row with m = 0 for an l > 0", _boundary, SCALED, 4,
                                      _search(_boundary(), 4, 3, boundary_rounds, "a boundary draw of a later trial"), 3),
        # sums past 32 bits
        "past_32_bits": _case("every P_l of round 1 is past 2^32", _three_far_values, NORMAL, 3, 1, 4),
        # the trial counts on one set (9 is the default of K = 1024)
        **{"trials_%d" % L: _case("L = %d" % L, lambda: _uniform(3000, 12, 7), SCALED, 12, 3, L) for L in (1, 2, 9, 16)},
        # block, segment and cap edges (sizes from the plan), K <= 4 so that the restatement stays fast
        "rows_block_minus": _case("rows just below a block", lambda: _uniform(B - 1, 3, 31), SCALED, 4, 0, 3),
        "rows_block": _case("rows = a block", lambda: _uniform(B, 3, 32), SCALED, 4, 0, 3),
        "rows_block_plus": _case("rows just above a block: a second segment of one row", lambda: _uniform(B + 1, 3, 33), NORMAL, 4,
                                 0, 3),
        "rows_segs_minus": _case("rows = 2 seg_rows - 1, candidates on both sides of a segment edge",
                                 lambda: _edge_rows(two_seg - 1), SCALED, 4,
                                 _search(_edge_rows(two_seg - 1), 4, 4, lambda r: edge_draws(two_seg - 1, r), "edge draws"), 4),
        "rows_segs_plus": _case("rows = 2 seg_rows + 1, candidates on both sides of a segment edge",
                                lambda: _edge_rows(two_seg + 1), NORMAL, 4,
                                _search(_edge_rows(two_seg + 1), 4, 4, lambda r: edge_draws(two_seg + 1, r), "edge draws"), 4),
        "rows_cap_minus": _case("rows = segments_cap * block - 1: every segment one block, the last a row short",
                                lambda: _uniform(S * B - 1, 3, 35, 0, 64), NORMAL, 3, 1, 3),
        "rows_cap_plus": _case("rows = segments_cap * block + 1: seg_rows exceeds one block",
                               lambda: _uniform(S * B + 1, 3, 36, 0, 64), SCALED, 3, 2, 3),
        "rows_select_wide": _case("seg_rows past the select's lanes: a lane of its row scan weighs two rows",
                                  lambda: _uniform(S * 1024 + 1, 1, 37, 0, 256), NORMAL, 3, 3, 3),
        # many seeds at the default trial count
        "k300": _case("K not a power of two, the default L = 7", lambda: _uniform(8257, 12, 42), NORMAL, 300, 6, 0),
        "k300_d48": _case("K not a power of two, D = 48, the default L = 7", lambda: _uniform(4097, 48, 43), SCALED, 300, 7, 0),
    }
    # every padded width 4 .. 64 with real bytes at the pad's ordinal, the colour spaces in turn, L = 2 or 3
    for i, dim in enumerate(WIDTH_DIMS):
        cs = (SCALED, NORMAL)[i % 2]
        t["width_%d" % dim] = _case("row width %d (%d words), real bytes at the pad's ordinal" % (dim, i + 1),
                                    functools.partial(_pad_valued, dim, cs), cs, 8, dim, 2 + i % 2)
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
def result(name):
    """The restatement's dict for the case: computed once, shared, read-only."""
    c = table()[name]
    r = ref.kmeanspp_greedy(rows(name), c["K"], c["seed"], c["trials"])
    for k in ("rows", "potential", "trial", "trial_rows", "trial_potential"):
        r[k].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def expected(name):
    """What Engine.kmeanspp_greedy returns for the case: (C, rows, potential, info)."""
    r = result(name)
    C = ref.codebook(rows(name), table()[name]["cs"], r["rows"], r["placed"])
    C.setflags(write=False)
    return C, r["rows"], r["potential"], {k: r[k] for k in ("placed", "trials", "trial", "trial_rows", "trial_potential")}
