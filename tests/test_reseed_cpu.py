"""QVQ_REFINE_RESEED without a GPU: the engine's host helpers (qvq_host_row_error,
qvq_host_reseed_far_key, qvq_host_reseed_select: the text the device passes run) against the numpy
restatement of tests/helpers/reseed_ref.py, the restatement against the committed trace, and the
CLI's --reseed argument errors."""
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT
from helpers import reseed_ref as ref

QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")


def far_keys(far, q):
    """The device's far-row keys of the helper's far rows (0: a cell without rows)."""
    return [quant_amd.host_reseed_far_key(int(q[r]), int(r)) if r >= 0 else 0 for r in far]


@pytest.mark.parametrize("cs", [ref.SCALED, ref.NORMAL])
@pytest.mark.parametrize("dim", [1, 3, 12, 13, 64])
def test_row_error_matches_restatement(cs, dim):
    rng = np.random.default_rng(dim * 2 + cs)
    tab = quant_amd.colorspace_values(cs)
    X = tab[rng.integers(0, 256, (40, dim))]
    # centroids as the engine forms them: means of table values, and the extremes of the range
    C = np.stack([tab[rng.integers(0, 256, (5, dim))].mean(axis=0) for _ in range(6)] +
                 [np.full(dim, tab.min()), np.full(dim, tab.max())])
    A = rng.integers(0, C.shape[0], 40).astype(np.uint32)
    want = ref.row_errors(X, C, A, cs)
    got = [quant_amd.host_row_error(X[i], C[A[i]], cs) for i in range(40)]
    assert got == [int(x) for x in want]
    assert max(got) < 1 << 31
    if dim == 64:   # the bound of the contract: e = 64 (SCALED), 64 * 255^2 (NORMAL), still below 2^31
        top = quant_amd.host_row_error(np.full(64, tab.max()), np.full(64, tab.min()), cs)
        assert top == (64 << 24 if cs == ref.SCALED else (64 * 255 * 255) << 8) and top < 1 << 31


def test_row_error_order_is_the_contracts():
    """A row whose error depends on the order of summation: ascending d, not a pairwise sum."""
    x = np.array([1.0, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27]) * 1.0
    c = np.zeros(5)
    e = 0.0
    for d in range(5):
        e = e + (x[d] - c[d]) * (x[d] - c[d])
    assert quant_amd.host_row_error(x, c, ref.SCALED) == int(np.floor(e * 2.0 ** 24))


def test_select_matches_restatement_on_random_cells():
    rng = np.random.default_rng(7)
    for trial in range(20):
        K, N = int(rng.integers(2, 40)), int(rng.integers(1, 200))
        A = rng.integers(0, K, N).astype(np.uint32)
        A[A % 3 == trial % 3] = A[0]                       # leave cells empty
        q = rng.integers(0, 6, N).astype(np.uint64)        # many equal errors and sums
        E, n, far = ref.cell_stats(q, A, K)
        empties, donors = ref.select(E, n)
        got_e, got_r = quant_amd.host_reseed_select(E, n, far_keys(far, q))
        assert got_e == empties and got_r == [int(far[d]) for d in donors], trial


def test_equal_sums_lower_cell_gives_first():
    E, n = [9, 0, 9, 9, 0], [2, 0, 2, 2, 0]
    keys = [quant_amd.host_reseed_far_key(1, r) for r in (10, 0, 20, 30, 0)]
    assert quant_amd.host_reseed_select(E, n, keys) == ([1, 4], [10, 20])
    assert ref.select(np.array(E, np.uint64), np.array(n, np.uint64)) == ([1, 4], [0, 2])


def test_equal_errors_lowest_row_wins():
    q = np.array([3, 7, 7, 1, 7], np.uint64)
    A = np.zeros(5, np.uint32)
    _, _, far = ref.cell_stats(q, A, 1)
    assert far[0] == 1
    keys = [quant_amd.host_reseed_far_key(int(q[r]), r) for r in range(5)]
    assert max(keys) == keys[1] and keys[1] == (7 << 32) | (0xFFFFFFFF - 1)
    assert quant_amd.host_reseed_select([25, 0], [5, 0], [max(keys), 0]) == ([1], [1])


def test_more_empties_than_donors():
    E, n = [0, 5, 0, 0, 8, 0], [0, 3, 0, 0, 2, 0]
    keys = [0, quant_amd.host_reseed_far_key(2, 11), 0, 0, quant_amd.host_reseed_far_key(4, 5), 0]
    assert quant_amd.host_reseed_select(E, n, keys) == ([0, 2], [5, 11])
    assert ref.select(np.array(E, np.uint64), np.array(n, np.uint64)) == ([0, 2], [4, 1])


def test_single_row_and_zero_error_cells_give_nothing():
    E, n = [50, 0, 0, 4], [1, 9, 0, 2]    # cell 0: one row; cell 1: E = 0; cell 3 the only donor
    keys = [quant_amd.host_reseed_far_key(50, 0), quant_amd.host_reseed_far_key(0, 1), 0,
            quant_amd.host_reseed_far_key(3, 8)]
    assert quant_amd.host_reseed_select(E, n, keys) == ([2], [8])
    assert quant_amd.host_reseed_select([50, 0, 0], [1, 9, 0], keys[:3]) == ([], [])


def test_reseed_grid_shape():
    g = quant_amd.host_reseed_grid()
    assert g["block"] % 64 == 0 and g["block"] >= 64 and g["blocks"] >= 1


def test_helper_reproduces_committed_trace():
    with open(os.path.join(GOLDEN, "refine_reseed_trace.json")) as f:
        want = json.load(f)
    got = ref.record()
    assert set(got) == set(want) == set(ref.CASES)
    for name, w in want.items():
        g = got[name]
        for key in ("iters", "stop", "changed", "reseeded", "empty_last"):
            assert g[key] == w[key], (name, key)
        assert g["distortion"] == pytest.approx(w["distortion"], rel=1e-12), name
        assert g["d_last"] == pytest.approx(w["d_last"], rel=1e-12), name
    # the figures the feature was specified with
    w = want["s128_b2_6_scaled"]
    assert w["reseeded"] == [4] + [0] * 21 and w["iters"] == 22 and w["stop"] == ref.STOP_FIXED
    assert abs(w["d_last"] - 0.0136582) < 5e-8 and w["empty_last"] == 0
    w = want["s96_b4_5_scaled"]
    assert w["reseeded"] == [1] + [0] * 9 and w["iters"] == 10 and w["stop"] == ref.STOP_FIXED
    for name in ("s64_b2_4_scaled", "s64_b2_4_normal", "s128_b2_6_normal"):
        assert not any(want[name]["reseeded"]), name
    assert want["s128_b2_10_scaled"]["reseeded"][:3] == [438, 5, 0]
    assert want["s128_b2_10_normal"]["reseeded"][:3] == [269, 4, 0]


def test_without_empties_the_loop_is_refine_refs():
    """s64_b2_4 never has an empty cell: the reseeding loop is the plain one."""
    from helpers import refine_ref
    X, start, (C, A, d, info) = ref.run_case("s64_b2_4_scaled")
    C_p, A_p, d_p, info_p = refine_ref.refine(X, *start, max_iters=100, eps=0.0)
    assert np.array_equal(C, C_p) and np.array_equal(A, A_p) and d == d_p
    assert info["changed"] == info_p["changed"] and info["stop"] == info_p["stop"]


@pytest.mark.parametrize("bad", [["--reseed"],                                   # needs --refine > 0
                                 ["--reseed", "--refine", "0"],
                                 ["--reseed", "--fresh"],
                                 ["--reseed=1", "--refine", "3"],                # takes no value
                                 ["--reseed", "--refine", "3", "-q", "1"]])      # needs LBG
def test_cli_rejects_bad_reseed_arguments(bad):
    if not os.path.exists(QUANT):
        pytest.fail("quant CLI not built (run __graft_entry__.build())")
    r = subprocess.run([QUANT, "in.ppm", "-o", "out.quant", *bad], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: quant" in r.stderr, (r.returncode, r.stderr)


def test_python_quantizer_rejects_reseed_without_refine():
    with pytest.raises(quant_amd.QVQError) as e:
        quant_amd.LBGQuantizer(reseed=True)
    assert e.value.status == 1
