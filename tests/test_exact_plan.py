"""The case tables of the exact-mode edge tests (tests/helpers/exact_cases.py, run by
tests/test_gpu_exact.py) held to the engine's dispatch and to what they claim, on the CPU
(DESIGN.md 6.4): every declared qvq_exact_plan field is what quant_amd.host_exact_plan answers; the
chunk cases make every chunk win rows and put duplicates across chunks where the kd-tree does not
give the lowest index; the near-tie cases fill the bands of the relative gap on both sides of the
engine's tie_rel, and above it the reference's kd-tree answer is the long-double argmin (the
engine's assumption when it keeps the fp64 argmin there); the chain cases' data shows a plain sum,
a reversed sum and a compensation restarted per tile in every multi-tile cell; and the oracle's
kd-tree gives what the compiled reference kd-tree gave (tests/golden/ref_nn_exact.json, recorded
by tests/helpers/record_ref_nn.py)."""
import json
import os

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN
from helpers import exact_cases as ex
from oracle import oracle
from test_oracle_golden import _check_vs_reference

with open(os.path.join(GOLDEN, "ref_nn_exact.json")) as _f:
    REF_NN = json.load(_f)


def _plan_errors(cases):
    bad = []
    for c in cases:
        plan = quant_amd.host_exact_plan(c["D"], c["K"])
        got = {f: plan[f] for f in c["plan"]}
        if got != c["plan"]:
            bad.append("%s: declared %s, host_exact_plan %s" % (c["key"], c["plan"], got))
    return bad


def test_cases_take_their_declared_paths():
    bad = _plan_errors(ex.CHUNK_CASES + ex.NEARTIE_CASES + ex.CHAIN_CASES)
    assert not bad, "\n".join(bad)


def test_helper_formulas_are_the_engines():
    """kc and T as the helper computes them (to size its cases) against the engine's constants, for
    every dimension exact mode takes; chunks == 1 exactly up to K = kc."""
    for D in range(1, 65):
        p = quant_amd.host_exact_plan(D, ex.kc_of(D))
        assert (p["kc"], p["tile_rows"], p["chunks"], p["last_chunk"]) == (ex.kc_of(D), ex.tile_rows_of(D), 1, p["kc"])
        assert p["templated"] == int(D in ex.TEMPLATED)
        p = quant_amd.host_exact_plan(D, ex.kc_of(D) + 1)
        assert (p["chunks"], p["last_chunk"]) == (2, 1)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.host_exact_plan(65, 4)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.host_exact_plan(12, 0)


def test_table_shape():
    """What the tables are meant to hold: every D at kc, kc + 1 and 2 kc + 1; D = 12 and 20 also at
    kc - 1, 2 kc and 3 kc - 7; the register-resident instantiations and the generic one; the tile
    sizes the chain cases name."""
    names = {(c["D"], c["K_name"]) for c in ex.CHUNK_CASES}
    for D in (3, 6, 12, 48, 1, 5, 20, 33, 63, 64):
        assert {(D, n) for n in ("kc", "kc+1", "2kc+1")} <= names
    for D in (12, 20):
        assert {(D, n) for n in ("kc-1", "2kc", "3kc-7")} <= names
    assert len(ex.CHUNK_CASES) == 36 and all(c["N"] == 777 for c in ex.CHUNK_CASES)
    assert ex.kc_of(1) == 8192 and ex.kc_of(64) == 128 and ex.kc_of(12) + 1 == 683 and ex.kc_of(48) + 1 == 171
    assert [c["plan"]["tile_rows"] for c in ex.CHAIN_CASES] == [4096, 341, 124, 85, 65, 64]
    assert len(ex.NEARTIE_CASES) == 12
    assert [c["N"] for c in ex.ROW_CASES[:8]] == [1, 2, 3, 37, 255, 256, 257, 1025]
    assert all((1 << c["bits"]) > c["N"] for c in ex.ROW_CASES if c["N"] <= 257)
    T = quant_amd.host_exact_plan(ex.MEAN_D, 1)["tile_rows"]
    assert sorted({c["N"] for c in ex.MEAN_CASES}) == [1, 2, T - 1, T, T + 1, 2 * T + 1]
    assert set(REF_NN["cases"]) == {c["key"] for c in ex.CHUNK_CASES + ex.NEARTIE_CASES}


@pytest.mark.parametrize("case", ex.CHUNK_CASES, ids=ex.key)
def test_chunk_case(case):
    X, C = ex.inputs(case)
    A = ex.oracle_nn(case).astype(np.int64)
    K, kc, chunks = case["K"], case["plan"]["kc"], case["plan"]["chunks"]
    assert X.shape == (case["N"], case["D"]) and C.shape == (K, case["D"])
    # what the codebook holds
    assert int(np.sum((C == 0).all(axis=1))) >= 2                       # zero vectors
    d = ex.sqdist(X, C)
    assert int(np.sum(d.min(axis=1) == 0)) >= min(K // 4, 50)            # rows with an exact copy: d1 = 0
    assert np.array_equal(C[K - 1], C[np.flatnonzero((C[: K - 1] == C[K - 1]).all(axis=1))[0]])
    if K > kc + 1:                                                       # k and k + kc (K - 1 is taken)
        n2 = min(kc, K - 1 - kc)
        same = (C[kc:kc + n2] == C[:n2]).all(axis=1) & (C[:n2] != 0).any(axis=1)
        assert int(same.sum()) >= ex.N_DUP - 1
    # from the oracle's answer alone
    won = set((A // kc).tolist())
    assert won == set(range(chunks)), "chunks that win a row: %s of %d" % (sorted(won), chunks)
    if chunks > 1:
        i1, i2 = ex.best_two(X, C)
        runner_up = np.where(A == i1, i2, i1)
        assert int(np.sum(A // kc > runner_up // kc)) >= 1, "no winner in a later chunk than its runner-up"
        cross = (A != i1) & (C[A] == C[i1]).all(axis=1) & (A // kc != i1 // kc)
        assert int(cross.sum()) >= 1, "no cross-chunk duplicate answered above the lowest tied index"
    _check_vs_reference(REF_NN["cases"][case["key"]], C, X, A, case["key"])


@pytest.mark.parametrize("case", ex.NEARTIE_CASES, ids=ex.key)
def test_neartie_case(case):
    X, C, pair = ex.inputs(case)
    A = ex.oracle_nn(case).astype(np.int64)
    kc = case["plan"]["kc"]
    assert (pair[:, 1] > pair[:, 0]).all()
    straddle = pair[:, 0] // kc != pair[:, 1] // kc
    if case["plan"]["chunks"] > 1:
        assert int(straddle.sum()) == (len(pair) // 2 if case["K"] > 2 * kc else 1)
        own = np.flatnonzero(pair[:, 1] == case["K"] - 1)               # the chunk of one belongs to a pair
        assert len(own) == 1
    # every row's two nearest code vectors are its own pair
    i1, i2 = ex.best_two(X, C)
    assert np.array_equal(np.sort(np.stack([i1, i2], axis=1), axis=1), pair)
    d_b, d_a, gap = ex.pair_gap(X, C, pair)
    counts = ex.band_counts(gap)
    print("rows per band of the relative gap:", counts)
    want = ex.bands_expected(case["offset"])
    assert any(b[1] <= ex.TIE_REL for b in want) and any(b[0] >= ex.TIE_REL for b in want)   # both sides
    short = [b for b in want if counts[b] < 5]
    assert not short, "bands of the relative gap with fewer than 5 rows: %s" % short
    assert int(np.sum((d_a < d_b) & (gap > ex.TIE_REL))) >= 8           # the nearer one at the higher index
    # the engine's assumption: past tie_rel the reference's answer is the argmin
    argmin = np.where(d_a < d_b, pair[:, 1], pair[:, 0])
    above = gap > ex.TIE_REL
    wrong = np.flatnonzero(above & (A != argmin))
    assert len(wrong) == 0, "kd-tree != long-double argmin at relative gaps %s" % gap[wrong][:8]
    if case["plan"]["chunks"] > 1:                                      # the chunk of one's row: no tie, the scan's
        assert above[own[0]] and A[own[0]] == case["K"] - 1
    # and within it the kd-tree does not always give the lower index: those rows need the tree
    assert int(np.sum(~above & (A == pair[:, 1]))) >= 5
    _check_vs_reference(REF_NN["cases"][case["key"]], C, X, A, case["key"])


@pytest.mark.parametrize("case", ex.CHAIN_CASES, ids=ex.key)
def test_chain_case(case):
    X, A = ex.inputs(case)
    T = quant_amd.host_exact_plan(case["D"], case["K"])["tile_rows"]
    sizes = ex.chain_sizes(T)
    assert np.array_equal(np.bincount(A, minlength=case["K"]), sizes)
    assert not np.array_equal(np.argsort(A, kind="stable"), np.arange(len(A)))
    ref = oracle.centroids(X, A, case["K"], sum_mode=0)
    for k, n in enumerate(sizes):
        if n <= T:
            continue
        V = X[A == k]
        np.testing.assert_array_equal(ex.kahan_mean(V), ref[k])          # the restatement used below
        for what, got in (("a plain sum", ex.plain_mean(V)), ("Kahan in reversed order", ex.kahan_mean(V[::-1])),
                          ("a compensation restarted every T rows", ex.kahan_mean(V, restart=T))):
            assert (got != ref[k]).any(), "%s: the cell of %d rows does not show %s" % (case["key"], n, what)


def test_stride_case_passes_every_grid_cap():
    g = quant_amd.host_exact_grids()
    for f in ("assign_blocks", "iota_blocks", "dist_blocks"):
        assert ex.STRIDE_CASE["N"] > g[f] * g["block"], f
    assert ex.STRIDE_CASE["N"] % g["block"] != 0
    assert all(c["N"] > 3 * g["block"] and c["N"] % g["block"] for c in ex.CHUNK_CASES)
