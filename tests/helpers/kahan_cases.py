"""The Kahan chain case table: each case is a set of (cell, component) chains given as ordinals
u = byte ^ 0x80 (value u / 255: 0 is u = 0, 1.0 is u = 255), laid out as rows with an assignment,
and the claim it exists for.  Chain (k, d) is component d of the rows with A == k in ascending row
order; the cells' rows are interleaved by a seeded shuffle of the cell labels that keeps each
cell's own order, so the device's stable sort does real work.

tests/test_kahan_cases_cpu.py measures every claim on the restatement of the device's evaluation
(tests/cpp/test_kahan_chain.cpp) and holds the constants below to quant_amd/csrc/kahan_par.hpp;
tests/test_gpu_kahan_cases.py runs the cases on the device against the oracle.

A claim is a list of checks (cell, component, line, field, op, value) on the restatement's
per-chain lines: line "KCHAIN" is the whole chain, "KSPLIT" the chain cut at the case's first
list of cuts; the fields are test_kahan_chain.cpp's struct Info."""
import functools

import numpy as np

# The sizes the cases were chosen for (kahan_par.hpp L, SPB, NE; k_kahan.hip kahan_direct_max's
# default and the grid cap of the meta / build kernels with their waves per workgroup).
L, SPB, NE, DIRECT_MAX = 64, 64, 16, 4096
BLK = L * SPB
GRID_CAP, WPB = 2048, 4
ROUTE_DIRECT, ROUTE_FUNCTIONS, ROUTE_CHAINED = 1, 2, 3   # quant_amd.KAHAN_ROUTE_*


def _rng(seed):
    return np.random.default_rng(seed)


# ---- the chain kinds of tests/cpp/test_kahan_chain.cpp (ordinals) ---------------------------------
def noise(n, seed):
    return _rng(seed).integers(0, 256, n)


def saturated(n, seed):
    r = _rng(seed)
    return np.where(r.integers(0, 4, n) == 0, 255, r.integers(0, 256, n))


def dark(n, seed):
    return _rng(seed).integers(0, 8, n)


def narrow(n, seed):
    r = _rng(seed)
    lo, span = int(r.integers(0, 256)), 1 + int(r.integers(0, 40))
    return np.minimum(255, lo + r.integers(0, span, n))


def zeros_heavy(n, seed):
    r = _rng(seed)
    return np.where(r.integers(0, 3, n) == 0, 0, r.integers(0, 256, n))


def flat_one(n, seed):
    return np.full(n, 255)


def one_and_mid(n, seed):
    r = _rng(seed)
    return np.where(r.integers(0, 2, n) == 1, 255, 128 + r.integers(0, 8, n))


def quarter(n, seed):
    return 64 + _rng(seed).integers(0, 64, n)


def regions2(period):
    def kind(n, seed):
        r = _rng(seed)
        return np.where((np.arange(n) // period) % 2 == 1, r.integers(0, 4, n), 128 + r.integers(0, 128, n))
    return kind


def regions3(period):
    def kind(n, seed):
        r = _rng(seed)
        ph = (np.arange(n) // period) % 3
        return np.where(ph == 0, 0, np.where(ph == 1, r.integers(0, 6, n), 255))
    return kind


KINDS = [noise, saturated, dark, narrow, zeros_heavy, flat_one, one_and_mid, quarter,
         regions2(64), regions2(100), regions2(4096), regions3(64), regions3(100), regions3(4096)]
MIXED = [noise, flat_one, dark, one_and_mid, zeros_heavy, saturated, regions2(100), quarter, regions3(64), narrow]


def values(u):
    """The SCALED values of ordinals u, as the reference forms them."""
    return (np.asarray(u, np.float64)) * (1.0 / 255)


def kahan_state(u, skip_zero_segments=False):
    """The reference's chain over ordinals u: (sum, c) after the last step (sumInArea's loop).
    skip_zero_segments: what an evaluation would compute that skipped every whole segment of zeros
    before the sum reaches 2 whatever c is -- wrong once c != 0, see _transient."""
    x = values(u).tolist()
    s, c, i, n = 0.0, 0.0, 0, len(x)
    while i < n:
        if skip_zero_segments and i % L == 0 and s < 2.0 and not np.any(u[i:i + L]):
            i += L
            continue
        y = x[i] - c
        t = s + y
        c = (t - s) - y
        s = t
        i += 1
    return s, c


class Case:
    """cells: {k: [D arrays of n_k ordinals]}; K cells in all (the others empty)."""

    def __init__(self, cells, K, D, route, checks=(), cuts=(), device=None, seed=1, totals=None):
        for ch in cells.values():
            assert len(ch) == D and len({len(c) for c in ch}) == 1
        self.cells, self.K, self.D, self.route = cells, K, D, route
        self.checks, self.cut_lists, self.device, self.seed = list(checks), [list(c) for c in cuts], device or {}, seed
        # device: claims on qvq_get_kahan_stats' counters (the restatement's totals over the chains
        # are the same numbers); totals: claims on totals only the restatement keeps
        self.totals = totals or {}

    @functools.cached_property
    def layout(self):
        """(codes [N, D] uint8 bytes, A [N] uint32)."""
        keys = sorted(self.cells)
        lens = [len(self.cells[k][0]) for k in keys]
        A = np.repeat(np.array(keys, np.uint32), lens)
        if len(keys) > 1:
            A = A[_rng(self.seed).permutation(A.size)]   # labels shuffled; a cell's rows stay in order
        codes = np.zeros((A.size, self.D), np.uint8)
        for k in keys:
            codes[A == k] = (np.stack(self.cells[k], 1).astype(np.uint8)) ^ 0x80
        return codes, A

    @property
    def n(self):
        return sum(len(ch[0]) for ch in self.cells.values())

    def row_of(self, k, p):
        """The row of cell k's step p (N for p = its length): a cut there is a cut before step p."""
        rows = np.flatnonzero(self.layout[1] == k)
        return int(rows[p]) if p < rows.size else int(rows[-1]) + 1 if p == rows.size and rows.size else 0

    def cuts(self):
        """The row cut lists (each from 0 to N, not decreasing)."""
        out = []
        for c in self.cut_lists:
            c = sorted(min(self.n, int(x)) for x in c)
            out.append(np.array([0] + c + [self.n], np.uint64))
        return out

    def chains(self):
        """[(k, d, ordinals, the cuts of cuts()[0] in the chain's own steps, or None)]."""
        _, A = self.layout
        cuts = self.cuts()
        out = []
        for k in sorted(self.cells):
            local = None
            if cuts:
                before = np.concatenate([[0], np.cumsum(A == k)])
                local = before[cuts[0].astype(np.int64)].astype(np.uint32)
            for d in range(self.D):
                out.append((k, d, np.asarray(self.cells[k][d], np.uint8), local))
        return out


def _cell(n, D, seed, kinds=MIXED):
    return [kinds[d % len(kinds)](n, seed * 100 + d) for d in range(D)]


def _noise_cell(n, D, seed):
    """Noise in the first six components, mixed kinds in the others."""
    return [(noise if d < 6 else MIXED[d % len(MIXED)])(n, seed * 100 + d) for d in range(D)]


SHORT = [1, 2, 63, 64, 65, 127, 128, 129]
LENGTHS = SHORT + [511, 512, 513, 4095, 4096]


def _lengths(extra=(), lens=LENGTHS, K_more=1):
    ls = list(lens) + list(extra)
    cells = {k: _noise_cell(n, 12, 10 + k) for k, n in enumerate(ls)}
    route = ROUTE_FUNCTIONS if max(ls) > DIRECT_MAX else ROUTE_DIRECT
    checks = []
    if route == ROUTE_FUNCTIONS:
        for k, n in enumerate(ls):
            checks += [(k, 0, "KCHAIN", "segs", "==", -(-n // L)), (k, 0, "KCHAIN", "blocks", "==", -(-n // BLK))]
    return Case(cells, len(ls) + K_more, 12, route, checks)   # (the last cell is empty)


def _lengths_small_cuts():
    c = _lengths(lens=SHORT)
    c.route = ROUTE_DIRECT
    return c


def _long(K):
    n = 64 * BLK + 1
    checks = [(0, 0, "KCHAIN", "blocks", "==", 65), (0, 0, "KCHAIN", "segs", "==", 64 * SPB + 1),
              (0, 0, "KCHAIN", "left", "==", 1)]
    return Case({0: [noise(n, 5)]}, K, 1, ROUTE_FUNCTIONS, checks,
                cuts=[[BLK - 1, BLK, BLK + 1, 63 * BLK, 64 * BLK, 64 * BLK + 1]])


def _kinds(n):
    cells = {0: [k(n, 300 + i) for i, k in enumerate(KINDS[:12])],
             1: [k(n, 320 + i) for i, k in enumerate(KINDS[12:] + MIXED)]}
    c = Case(cells, 3, 12, ROUTE_FUNCTIONS, seed=n)
    # (totals over the case's chains; the device's counters of the same call)
    c.device = {"block_misses": (">", 0), "replays": (">", 0), "blocks_not_composable": (">", 0)}
    # cuts: empty first and last rank, a repeated cut, inside the transient of cell 0's chains (a few
    # steps in), and around cell 0's first segment and block boundaries
    c.cut_lists = [[0, c.row_of(0, 2), c.row_of(0, 2), c.row_of(0, L - 1), c.row_of(0, L), c.row_of(0, L + 1),
                    c.row_of(0, BLK - 1), c.row_of(0, BLK), c.row_of(0, BLK + 1), c.n],
                   [c.row_of(1, 1), c.row_of(1, BLK)]]
    flat, one_mid = 5, 6
    c.checks = [
        (0, flat, "KCHAIN", "tau", "==", 2), (0, flat, "KCHAIN", "left", "==", 1),
        # flat 1.0: every step a decision; the functions answer or are replayed, the bits hold (ok)
        (0, 0, "KCHAIN", "blocks", "==", -(-n // BLK)),
        (0, 2, "KCHAIN", "left", "==", 1),
    ]
    return c


# ---- the transient ---------------------------------------------------------------------------------
NT = 5000                # rows of the transient cell: past DIRECT_MAX, so the functions run
ZLEAD = BLK + 70         # a run of zeros longer than a block
TWO_ONES = [62, 63, 64, 4094, 4095, 4096]
C_PREFIX = [128, 128, 128, 77]   # leaves c != 0 with sum < 2 (asserted in _transient)


def _two_ones(second):
    u = np.zeros(NT, np.int64)
    u[5] = u[second] = 255
    return u


# Where a zero step is not idle: after ordinals (a, b) with b's value above the sum so far, c is
# not the step's exact error but a whole ulp of the sum, and the next zero step folds it into the
# sum.  sum - c stays, but a following value d then rounds differently -- and a chain that ends on
# d shows it in its last bit.  So: zeros, (a, b) ending a segment, whole segments of zeros (more
# than a block), d as the last row.  An evaluation that skips those zeros because they are zeros
# (not looking at c) returns another sum; _transient asserts that for every triple.
FOLD = [(1, 34, 64), (1, 42, 64), (1, 34, 65), (1, 42, 66), (1, 34, 67), (1, 50, 64)]
NF = 78 * L + 1          # rows of the cell of these chains: d opens the last segment and ends the chain


def _fold(a, b, d):
    u = np.zeros(NF, np.int64)
    u[L - 2], u[L - 1], u[NF - 1] = a, b, d
    return u


def _below2():
    """5000 rows whose total stays below 2: small values far apart, inexact steps from sum >= 1."""
    u = np.zeros(NT, np.int64)
    u[::50] = _rng(9).integers(1, 5, len(u[::50]))      # 100 values of at most 4 / 255
    u[7] = 200
    return u


def _transient():
    s, c = kahan_state(C_PREFIX)
    assert c != 0.0 and s < 2.0, (s, c)
    lead = np.concatenate([np.zeros(ZLEAD, np.int64), noise(NT - ZLEAD, 41)])
    cpre = np.concatenate([C_PREFIX, np.zeros(ZLEAD, np.int64), noise(NT - ZLEAD - len(C_PREFIX), 42)])
    # the same with the prefix ending on a segment boundary: the zeros start a segment with c != 0
    cpre64 = np.concatenate([np.zeros(L - len(C_PREFIX), np.int64), C_PREFIX, np.zeros(ZLEAD, np.int64),
                             noise(NT - ZLEAD - L, 43)])
    assert kahan_state(_below2())[0] < 2.0
    chains = [np.zeros(NT, np.int64), lead, cpre, cpre64, _below2()] + [_two_ones(p) for p in TWO_ONES] + [noise(NT, 44)]
    first_nz = ZLEAD // L * L   # the segment holding the first value after the zeros
    checks = [
        (0, 0, "KCHAIN", "left", "==", 0), (0, 0, "KCHAIN", "segs", "==", -(-NT // L)),
        # leading zeros longer than a block: skipped while c = 0, a whole block and then segments
        (0, 1, "KCHAIN", "skipped", "==", ZLEAD // L), (0, 1, "KCHAIN", "left", "==", 1),
        (0, 1, "KCHAIN", "tau", ">", ZLEAD),
        # zeros after a rounding step: not skipped, stepped through with c != 0
        (0, 2, "KCHAIN", "skipped", "==", 0), (0, 2, "KCHAIN", "held", ">=", ZLEAD // L - 1),
        (0, 2, "KCHAIN", "tau", ">", ZLEAD),
        (0, 3, "KCHAIN", "skipped", "==", 0), (0, 3, "KCHAIN", "held", ">=", ZLEAD // L),
        (0, 3, "KCHAIN", "tau", ">", ZLEAD),
        # never leaves the transient: total below 2 on a chain longer than a block
        (0, 4, "KCHAIN", "left", "==", 0), (0, 4, "KCHAIN", "tau", "==", NT),
    ]
    for i, p in enumerate(TWO_ONES):   # the sum reaches 2 on step p: the transient ends at p + 1
        checks += [(0, 5 + i, "KCHAIN", "tau", "==", p + 1), (0, 5 + i, "KCHAIN", "left", "==", 1),
                   (0, 5 + i, "KCHAIN", "treplay", "==", int((p + 1) % L != 0))]
    # the first list of cuts: inside the prefix (c != 0 handed to a rank of zeros only), on the
    # steps where sums reach 2, at segment and block boundaries +- 1
    cuts = [[len(C_PREFIX), L, L + 1, 2 * L, BLK - 1, BLK, BLK + 1, ZLEAD, ZLEAD + 1],
            [0, 0, NT, NT], [2, 2, 62, 63, 64, 65], [4094, 4095, 4096, 4097], [first_nz, first_nz + L]]
    checks += [
        # the rank [len(C_PREFIX), L) of chain 2 holds zeros only and enters with c != 0, sum < 2
        (0, 2, "KSPLIT", "gate_c", ">", 0), (0, 3, "KSPLIT", "gate_c", ">", 0),
        (0, 0, "KSPLIT", "gate_c", "==", 0),
    ]
    folds = [_fold(*t) for t in FOLD]
    for u in folds:
        s, c = kahan_state(u[:L])
        assert c != 0.0 and s < 2.0 and kahan_state(u)[0] != kahan_state(u, skip_zero_segments=True)[0], u[u != 0]
        assert NF - 1 - L > BLK
    D = len(chains)
    cell1 = folds + [noise(NF, 45 + i) for i in range(D - len(folds))]
    # the first segment of zeros is stepped through with c != 0 (its first step folds c into the sum);
    # the others are skipped with c = 0; the chain ends below 2
    for d in range(len(folds)):
        checks += [(1, d, "KCHAIN", "held", "==", 1), (1, d, "KCHAIN", "skipped", "==", NF // L - 2),
                   (1, d, "KCHAIN", "left", "==", 0), (1, d, "KSPLIT", "gate_c", ">", 0)]
    c = Case({0: chains, 1: cell1}, 3, D, ROUTE_FUNCTIONS, checks, seed=3)
    # cuts in cell 0's steps (above), and one list in cell 1's: a rank of its zeros only, entered with c != 0
    c.cut_lists = [[c.row_of(0, p) for p in cuts[0]] + [c.row_of(1, L), c.row_of(1, NF - 1)]] + \
                  [[c.row_of(0, p) for p in cl] for cl in cuts[1:]] + [[c.row_of(1, L), c.row_of(1, NF - 1)]]
    return c


def _alignment():
    extra = [0, 1, 2, 3, 5, 6, 7, 9, 10]
    cells = {k: _cell(DIRECT_MAX + 1 + e, 5, 50 + k) for k, e in enumerate(extra)}
    c = Case(cells, 9, 5, ROUTE_FUNCTIONS)
    assert {(sum(DIRECT_MAX + 1 + e for e in extra[:k])) % 4 for k in range(9)} == {0, 1, 2, 3}
    return c


def _widths(D):
    def build():
        cells = {0: _cell(DIRECT_MAX + 1, D, 60 + D), 1: _cell(130, D, 61 + D)}
        return Case(cells, 3, D, ROUTE_FUNCTIONS, [(0, D - 1, "KCHAIN", "blocks", "==", 2)],
                    cuts=[[130, 131, BLK + 7]], seed=D)
    return build


def _grid_stride():
    D, cells = 48, {}
    for k in range(200):
        cells[k + (k >= 100)] = _cell(DIRECT_MAX + 1 if k == 17 else 1 + (k * 7) % 40, D, 70 + k)   # (cell 100 empty)
    c = Case(cells, 202, D, ROUTE_FUNCTIONS)
    assert (200 + 1) * D > GRID_CAP * WPB   # the (component, block) pairs pass the grid
    return c


def _many_long():
    """The walk enters block 0 inside (the transient ends in its first segments) and leaves it by an
    8-segment hit: only there must the evaluation fetch the next block's function itself.  Many such
    chains, since what a missing fetch leaves in its place is arbitrary."""
    D, K = 48, 96
    cells = {k: _cell(DIRECT_MAX + 1 + k % 8, D, 500 + k) for k in range(K)}
    return Case(cells, K + 1, D, ROUTE_FUNCTIONS, totals={"edge8": (">", 2000)}, seed=7)


# name -> (claim, builder).  Sizes: the smallest that still reach the branch.
CASES = {
    "lengths_direct": ("one cell per length at the segment, sub-block and block edges, all <= 4096: the "
                       "step-by-step kernel", lambda: _lengths()),
    "lengths_functions": ("the same cells and one of 4097 rows: the functions run for every cell",
                          lambda: _lengths([DIRECT_MAX + 1])),
    "lengths_blocks": ("8191, 8192, 8193 rows: the second block's edge", lambda: _lengths(lens=[8191, 8192, 8193])),
    "lengths_short_cuts": ("the cells of at most 129 rows, for two ranks at every cut", _lengths_small_cuts),
    "long_scatter": ("64 * 4096 + 1 rows in one cell, K = 2: the block scan's second trip and carry, the scatter",
                     lambda: _long(2)),
    "long_transpose": ("its K = 1 twin: the transpose", lambda: _long(1)),
    "kinds_4134": ("the ten kinds, regions at period 64, 100, 4096, chains of 4097 + 37 rows", lambda: _kinds(4134)),
    "kinds_12289": ("the same at 3 * 4096 + 1 rows", lambda: _kinds(3 * BLK + 1)),
    "transient": ("zeros, leading zeros past a block, zeros after a rounding step, sums reaching 2 at the "
                  "segment and block edges, a total below 2", _transient),
    "alignment": ("K = 9 cells of 4097 + {0,1,2,3,5,6,7,9,10} rows, D = 5: every koff % 4 before a long chain",
                  _alignment),
    "many_long": ("96 cells of 4097.. rows at D = 48: thousands of 8-segment hits that end a block entered inside",
                  _many_long),
    "grid_stride": ("200 cells at D = 48, one of 4097 rows: more (component, block) pairs than the grid",
                    _grid_stride),
}
for _D in (1, 5, 13, 27, 63, 64):
    CASES["width_%d" % _D] = ("D = %d through the functions: 4097 rows, 130 rows, an empty cell" % _D, _widths(_D))


# The cases with cuts, as a literal: collecting the GPU module then builds no case
# (test_kahan_cases_cpu.py holds it to the table).
SPLIT_CASES = ("long_scatter", "long_transpose", "kinds_4134", "kinds_12289", "transient",
               "width_1", "width_5", "width_13", "width_27", "width_63", "width_64")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][1]()
