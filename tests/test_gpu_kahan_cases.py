"""The Kahan centroid kernels (quant_amd/csrc/k_kahan.hip) on constructed chains and at large K.

Every case of tests/helpers/kahan_cases.py (its claims are measured on the CPU restatement by
tests/test_kahan_cases_cpu.py) runs through qvq_update_kahan and, at the case's cuts, through
qvq_update_kahan_split; the centroids must be the oracle's sequential Kahan chains (sumInArea,
src/Quantizer.cpp:59-87) bit for bit -- uint64 views, no tolerance.  qvq_get_kahan_stats says which
route the call took; the counters are asserted only where a case's claim names them."""
import functools

import numpy as np
import pytest

from helpers import kahan_cases as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

OPS = {"==": lambda a, b: a == b, ">": lambda a, b: a > b}


@functools.lru_cache(maxsize=None)
def _input(name, cs=oracle.SCALED):
    """(X, A, K, the oracle's Kahan centroids as bits): computed once, shared, read-only."""
    c = kc.case(name)
    codes, A = c.layout
    X = oracle.lut(cs)[codes]
    ref = oracle.centroids(X, A, c.K, sum_mode=0).view(np.uint64)
    for a in (X, A, ref):
        a.setflags(write=False)
    return X, A, c.K, ref


def _load(engine, X):
    import quant_amd
    engine.set_vectors(X)
    info = engine.training_info()
    assert info["mode"] == quant_amd.MODE_BYTE and info["colorspace"] == quant_amd.SCALED, info


def _empty_cells_are_zero(C, A, K):
    empty = np.setdiff1d(np.arange(K), A)
    assert not C.view(np.uint64)[empty].any()   # +0.0 in every component


@pytest.mark.parametrize("name", list(kc.CASES))
def test_case_is_the_reference_bits(engine, name):
    c = kc.case(name)
    X, A, K, ref = _input(name)
    _load(engine, X)
    C = engine.update_kahan(A, K)
    st = engine.kahan_stats()
    print(name, st)
    np.testing.assert_array_equal(C.view(np.uint64), ref)
    _empty_cells_are_zero(C, A, K)
    assert st["route"] == c.route, st
    if c.route == kc.ROUTE_DIRECT:   # the step-by-step kernel keeps no counters
        assert (st["blocks_not_composable"], st["block_misses"], st["replays"]) == (0, 0, 0), st
    for key, (op, val) in c.device.items():
        assert OPS[op](st[key], val), (name, key, st)


@pytest.mark.parametrize("name", kc.SPLIT_CASES)
def test_case_split_is_the_reference_bits(engine, name):
    c = kc.case(name)
    X, A, K, ref = _input(name)
    _load(engine, X)
    for cuts in c.cuts():
        C = engine.update_kahan_split(A, K, cuts)
        np.testing.assert_array_equal(C.view(np.uint64), ref, err_msg="cuts %s" % cuts.tolist())
        _empty_cells_are_zero(C, A, K)
    assert engine.kahan_stats()["route"] == kc.ROUTE_CHAINED


def test_two_ranks_at_every_cut_of_the_short_cells(engine):
    X, A, K, ref = _input("lengths_short_cuts")
    _load(engine, X)
    n = X.shape[0]
    bad = [p for p in range(n + 1)
           if not np.array_equal(engine.update_kahan_split(A, K, np.array([0, p, n], np.uint64)).view(np.uint64), ref)]
    assert not bad, bad


def test_normal_twin_returns_qvq_update(engine):
    """NORMAL values are integers, the exact sums are the Kahan sums: qvq_update_kahan documents
    qvq_update's route, and both are the oracle's chain."""
    import quant_amd
    X, A, K, ref = _input("lengths_direct", oracle.NORMAL)
    engine.set_vectors(X)
    assert engine.training_info()["colorspace"] == quant_amd.NORMAL
    C = engine.update_kahan(A, K)
    C_u, cnt = engine.update(A, K)
    np.testing.assert_array_equal(C.view(np.uint64), C_u.view(np.uint64))
    np.testing.assert_array_equal(C.view(np.uint64), ref)
    np.testing.assert_array_equal(cnt, np.bincount(A, minlength=K))


# ---- large K: the sort's key windows -----------------------------------------------------------------
LARGE_N = 3001


@functools.lru_cache(maxsize=None)
def _large_rows():
    X = oracle.lut(oracle.SCALED)[np.random.default_rng(11).integers(0, 256, (LARGE_N, 3)).astype(np.uint8)]
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("K", [16384, 16385, 40960, 40961, 65536, 1 << 20])
def test_large_k(engine, K):
    """Most cells empty, rows of both ends of the key range and of both sides of every window's
    edge; several rows in some cells (a chain of more than one step)."""
    import quant_amd
    plan = quant_amd.host_kahan_sort_plan(K)
    rng = np.random.default_rng(K)
    A = rng.integers(0, K, LARGE_N).astype(np.uint32)
    A[rng.integers(0, LARGE_N, 600)] = rng.integers(0, 20, 600) * (K // 20)     # repeated cells
    edges = [0, K - 1] + [w * plan["window_keys"] + o for w in range(1, plan["windows"]) for o in (-1, 0)]
    A[rng.choice(LARGE_N, 4 * len(edges), replace=False)] = np.repeat(np.array(edges, np.uint32), 4)
    X = _large_rows()
    ref = oracle.centroids(X, A, K, sum_mode=0).view(np.uint64)
    _load(engine, X)
    C = engine.update_kahan(A, K)
    assert engine.kahan_stats()["route"] == kc.ROUTE_DIRECT
    np.testing.assert_array_equal(C.view(np.uint64), ref)
    C = engine.update_kahan_split(A, K, np.array([0, 1000, 1000 + 64 * 15 + 1, LARGE_N], np.uint64))
    np.testing.assert_array_equal(C.view(np.uint64), ref)
