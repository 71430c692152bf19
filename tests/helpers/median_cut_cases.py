"""The median-cut case table: each case is a set of row ordinals u [N, dim], a colour space, a level
count and the claim it exists for.  tests/test_median_cut_cpu.py measures every claim on the
restatement (tests/helpers/median_cut_ref.py) and holds the sizes to qvq_host_median_cut_plan;
tests/test_gpu_median_cut.py runs the cases on the device."""
import functools

import numpy as np

NORMAL, SCALED = 0, 1
# The launch shape the sizes below were chosen for; test_median_cut_cpu.py compares it with
# quant_amd.host_median_cut_plan, so a change of the plan fails there and not silently here.
BLOCK, CAP, LDS_WORDS, MAX_GROUPS = 256, 768, 12288, 16


def _rng(seed):
    return np.random.default_rng(seed)


def _uniform(n, dim, seed, lo=0, hi=256):
    return _rng(seed).integers(lo, hi, (n, dim))


def _col(vals, dim=3, axis=0, fill=7):
    """Rows constant but for one component, which takes vals."""
    u = np.full((len(vals), dim), fill, np.int64)
    u[:, axis] = vals
    return u


def _skewed(n=2049, dim=12):
    # (2048 equal rows in one box: fl(1 / 2048) is exact, so is the centroid, and the distortion is 0)
    u = np.tile(_uniform(1, dim, 5), (n, 1))
    u[1777] = (u[1777] + 90) % 256
    return u


def _axis_tie(dim):
    u = _uniform(500, dim, 40 + dim, 100, 120)
    u[:, 0] = _rng(1).integers(10, 211, 500)
    u[:, dim - 1] = _rng(2).integers(30, 231, 500)
    u[0, 0], u[1, 0] = 10, 210          # range 200 in component 0 ...
    u[2, dim - 1], u[3, dim - 1] = 30, 230   # ... and in the last one
    return u


def _signed(dim=3):
    """Ordinals 0 (byte 0x80) and 255 (byte 0x7F) on the cut axis, and both sides of byte 0x00 / 0xFF
    (127, 128): raw-byte order would put 128..255 below 0..127."""
    v = np.concatenate([np.arange(0, 256, 5), [0, 255, 127, 128, 126, 129, 255, 0]])
    u = _uniform(len(v), dim, 77, 100, 110)
    u[:, 1] = v
    return u


# name -> (claim, builder of u, colour space, bits).  The cases whose distortion is exactly 0 are
# NORMAL with box sizes whose reciprocal is exact: integer centroids, so the direct sum and the
# device's closed form are both exactly 0.
CASES = {
    "one_row": ("N = 1: no box is ever cut", lambda: _uniform(1, 3, 1), NORMAL, 3),
    "two_rows": ("N = 2: one cut, then single rows", lambda: _col([9, 200]), NORMAL, 3),
    "all_equal": ("all rows equal: every cuts entry 0", lambda: np.tile(_uniform(1, 12, 2), (1024, 1)), NORMAL, 4),
    "bits0": ("bits = 0: one box, the mean", lambda: _uniform(300, 5, 3), SCALED, 0),
    "more_boxes_than_rows": ("N = 5 at bits = 4: empty boxes", lambda: _uniform(5, 3, 4), NORMAL, 4),
    "signed_bytes": ("bytes 0x7F (u = 255) and 0x80 (u = 0) on the cut axis", _signed, SCALED, 4),
    "signed_bytes_normal": ("the same ordinals as NORMAL values", _signed, NORMAL, 4),
    "axis_tie_d3": ("equal ranges in dims 0 and dim - 1: the lowest wins", lambda: _axis_tie(3), SCALED, 1),
    "axis_tie_d12": ("equal ranges in dims 0 and dim - 1: the lowest wins", lambda: _axis_tie(12), NORMAL, 1),
    "balance_tie_even": ("tie in the balance, even n_b", lambda: _col([1, 2, 2, 3]), SCALED, 1),
    "balance_tie_odd": ("tie in the balance, odd n_b", lambda: _col([1, 1, 2, 3, 3]), SCALED, 1),
    "cut_at_lo": ("boundary at lo", lambda: _col([4, 4, 9, 13]), NORMAL, 1),
    "cut_at_hi_minus_1": ("boundary at hi - 1", lambda: _col([0, 4, 4, 5, 5, 5]), SCALED, 1),
    "row_at_t": ("a row exactly at t stays low", lambda: _col([3, 8, 8, 8, 20, 30, 31]), SCALED, 1),
    "one_box_per_row": ("distinct rows, N = K: one row per box", lambda: _col(np.arange(64) * 3, dim=5, axis=2), NORMAL, 6),
    "skewed": ("all rows but one in one box", _skewed, NORMAL, 3),
    # row widths: every pad width class (pads 3, 1, 3, 0, 0, 0)
    "dim1": ("row width 1", lambda: _uniform(900, 1, 11), SCALED, 5),
    "dim3": ("row width 3", lambda: _uniform(900, 3, 13), NORMAL, 5),
    "dim5": ("row width 5", lambda: _uniform(900, 5, 15), SCALED, 5),
    "dim12": ("row width 12", lambda: _uniform(900, 12, 17), NORMAL, 5),
    "dim48": ("row width 48", lambda: _uniform(900, 48, 19), SCALED, 5),
    "dim64": ("row width 64", lambda: _uniform(900, 64, 21), NORMAL, 5),
    # pass edges (both row passes share block and cap)
    "rows_block_minus": ("rows just below a block", lambda: _uniform(BLOCK - 1, 3, 31), SCALED, 3),
    "rows_block": ("rows = a block", lambda: _uniform(BLOCK, 3, 32), SCALED, 3),
    "rows_block_plus": ("rows just above a block", lambda: _uniform(BLOCK + 1, 3, 33), SCALED, 3),
    "rows_cap_minus": ("rows just below block * cap", lambda: _uniform(BLOCK * CAP - 1, 3, 34), SCALED, 2),
    "rows_cap": ("rows = block * cap", lambda: _uniform(BLOCK * CAP, 3, 35), SCALED, 2),
    "rows_cap_plus": ("rows above block * cap: the loop's second trip", lambda: _uniform(BLOCK * CAP + 300, 3, 36), NORMAL, 2),
    # privatisation edges.  A pass keeps its per-box state in a block's LDS (LDS_WORDS words: 256 a box
    # for the histogram, 2 * dim for the ranges), in up to MAX_GROUPS groups of boxes, then in global
    # memory.  (dim, bits) whose last level's boxes 2^(bits-1) lie on both sides of each boundary:
    #   histogram      1 | 2 groups at 32 | 64 boxes;  16 groups | global at 512 | 1024
    #   ranges dim 12  1 | 2 groups at 512 | 1024;     16 groups | global at 8192 | 16384
    #   ranges dim 48  1 | 2 groups at 128 | 256;      16 groups | global at 2048 | 4096
    #   ranges dim 64                                  16 groups | global at 1024 | 2048
    #   ranges dim 3   1 | 2 groups at 2048 | 4096
    # and one level further on the global path at dim 12 and dim 48.  The rows are enough for the
    # last level to cut boxes.
    "hist_one_group": ("histogram: the last level in one block's LDS", lambda: _uniform(3000, 12, 51), SCALED, 6),
    "hist_two_groups": ("histogram: the first level in groups", lambda: _uniform(3000, 12, 52), SCALED, 7),
    "range_one_group_d12": ("ranges, dim 12: one group; histogram: the last level in LDS (16 groups)",
                            lambda: _uniform(6000, 12, 53), SCALED, 10),
    "range_two_groups_d12": ("ranges, dim 12: two groups; histogram: the first level in global memory",
                             lambda: _uniform(6000, 12, 54), NORMAL, 11),
    "range_four_groups_d12": ("ranges, dim 12: four groups; histogram: one level past",
                              lambda: _uniform(6000, 12, 55), SCALED, 12),
    "range_groups_last_d12": ("ranges, dim 12: the last level in LDS (16 groups)", lambda: _uniform(30000, 12, 61), SCALED, 14),
    "range_global_first_d12": ("ranges, dim 12: the first level in global memory", lambda: _uniform(50000, 12, 62), NORMAL, 15),
    "range_global_second_d12": ("ranges, dim 12: one level past", lambda: _uniform(80000, 12, 63), SCALED, 16),
    "range_one_group_d48": ("ranges, dim 48: one group", lambda: _uniform(3000, 48, 56), SCALED, 8),
    "range_two_groups_d48": ("ranges, dim 48: two groups", lambda: _uniform(3000, 48, 57), NORMAL, 9),
    "range_groups_last_d48": ("ranges, dim 48: the last level in LDS (16 groups)", lambda: _uniform(8000, 48, 58), SCALED, 12),
    "range_global_first_d48": ("ranges, dim 48: the first level in global memory", lambda: _uniform(14000, 48, 64), NORMAL, 13),
    "range_global_second_d48": ("ranges, dim 48: one level past", lambda: _uniform(24000, 48, 65), SCALED, 14),
    "range_groups_last_d64": ("ranges, dim 64: the last level in LDS (16 groups)", lambda: _uniform(4000, 64, 66), SCALED, 11),
    "range_global_first_d64": ("ranges, dim 64: the first level in global memory", lambda: _uniform(7000, 64, 67), NORMAL, 12),
    "range_one_group_d3": ("ranges, dim 3: one group", lambda: _uniform(9000, 3, 59), SCALED, 12),
    "range_two_groups_d3": ("ranges, dim 3: two groups", lambda: _uniform(9000, 3, 60), SCALED, 13),
}


@functools.lru_cache(maxsize=None)
def rows(name):
    u = np.ascontiguousarray(CASES[name][1](), dtype=np.int64)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def trace(name):
    """The restatement's (A, cuts, trace) for the case: computed once, shared."""
    from helpers import median_cut_ref as ref
    return ref.median_cut(rows(name), CASES[name][3])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's (C, A, distortion, cuts) for the case: computed once, shared."""
    from helpers import median_cut_ref as ref
    from oracle import oracle
    _, _, cs, bits = CASES[name]
    X = ref.values(rows(name), cs)
    A, cuts, _ = trace(name)
    C = oracle.centroids(X, A, 1 << bits, sum_mode=1)
    return C, A, ref.distortion(X, C, A), cuts
