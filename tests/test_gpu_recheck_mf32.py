"""recheck_mf32_kernel (the D = 12, K >= 512 recheck of flagged rows on the MFMA scores) at the edges of
its tile sweep, hit masks, candidate lists and row groups: tests/helpers/recheck_mf32_cases.py builds
the codebooks and rows, tests/test_recheck_mf32_cases.py holds them to their claims on the CPU.

Reference: oracle.kdtree_nn (the reference's kd-tree answer) for qvq_assign's indices, bit for bit,
and oracle.centroids(sum_mode=1) for the codebook after one qvq_refine step, whose fused sums take
the rows the recheck moves through the correction slabs.  Every constructed row must also have been
flagged by the search (timings()["flagged"]), so that it was the recheck that answered for it."""
import functools

import numpy as np
import pytest

from helpers import recheck_mf32_cases as rc
from oracle import oracle

pytestmark = pytest.mark.gpu
CODEBOOKS = [(K, cs) for K in rc.KS for cs in ("scaled", "normal")]


def _id(p):
    return "K%d-%s" % p


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


@functools.lru_cache(maxsize=None)
def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _reference(C, X):
    """oracle.kdtree_nn of every row, computed once per distinct row."""
    rows, inv = np.unique(X, axis=0, return_inverse=True)
    return oracle.kdtree_nn(C, rows)[inv.ravel()]


@functools.lru_cache(maxsize=None)
def _edges(K, cs):
    X, C, at = rc.edges(K, cs)
    want = _reference(C, X)
    want.setflags(write=False)
    return X, C, at, want


def _explain(K, cs, at, A, want):
    names = dict(zip(at.tolist(), rc.site_row_names(K, cs)))
    bad = np.flatnonzero(A != want)
    return "\n".join("row %d (%s): got %d, reference %d" % (r, names.get(int(r), "background"), A[r], want[r])
                     for r in bad[:30])


@pytest.mark.parametrize("K,cs", CODEBOOKS, ids=map(_id, CODEBOOKS))
def test_assign_edges(engine, K, cs):
    """Near ties in one tile, across the first and the last tile, across the lane halves and in the last
    tile; exact ties; 16, 17 and 40 equidistant code vectors in one half, both halves and many tiles; a
    row on a code vector."""
    X, C, at, want = _edges(K, cs)
    engine.set_vectors(X)
    A = engine.assign(C)
    t = engine.timings()
    print("flagged", t["flagged"][0], "constructed", len(at), "kd-tree rows", t["host_ties"][0])
    assert np.array_equal(A, want), _explain(K, cs, at, A, want)
    # the background rows lie on their own code vectors, far from every other: only the sites' rows
    assert t["flagged"][0] == len(at)
    # the midpoint rows and the cap sites' rows are ties for the reference
    ties = sum(1 for n in rc.site_row_names(K, cs) if n.startswith("cap:")) + 4
    assert t["host_ties"][0] >= ties


@pytest.mark.parametrize("K,cs", CODEBOOKS, ids=map(_id, CODEBOOKS))
def test_refine_one_step_edges(engine, K, cs):
    """One Lloyd step from the same codebook: the pruned, fused search, and the rows the recheck and the
    kd walk re-assign moved between the cells' sums."""
    X, C, at, want = _edges(K, cs)
    engine.set_vectors(X)
    C_r, A, _, info = engine.refine(K, C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1
    assert np.array_equal(A, want), _explain(K, cs, at, A, want)
    assert np.array_equal(C_r, oracle.centroids(X, want, K, sum_mode=1))


@pytest.mark.parametrize("name", rc.COUNT_NAMES)
@pytest.mark.parametrize("K,cs", rc.COUNT_CODEBOOKS, ids=map(_id, rc.COUNT_CODEBOOKS))
def test_assign_group_counts(engine, K, cs, name):
    """1, 31, 32, 33 flagged rows, the first group of wave 1 and a wave's second trip (its lists used
    again), on this device's grid."""
    n = rc.group_counts(_cu_count())[name]
    X, C = rc.counted(K, cs, n)
    want = _reference(C, X)
    engine.set_vectors(X)
    A = engine.assign(C)
    t = engine.timings()
    print("rows", len(X), "flagged", t["flagged"][0], "kd-tree rows", t["host_ties"][0])
    assert np.array_equal(A, want), "%d rows differ" % int(np.sum(A != want))
    assert t["flagged"][0] == n
    assert t["host_ties"][0] == n      # the midpoint of a mirrored pair: every copy is the kd-tree's


@pytest.mark.parametrize("K,cs", rc.COUNT_CODEBOOKS, ids=map(_id, rc.COUNT_CODEBOOKS))
def test_refine_one_step_second_trip(engine, K, cs):
    n = rc.group_counts(_cu_count())["second_trip"]
    X, C = rc.counted(K, cs, n)
    want = _reference(C, X)
    engine.set_vectors(X)
    C_r, A, _, info = engine.refine(K, C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1
    assert np.array_equal(A, want), "%d rows differ" % int(np.sum(A != want))
    assert np.array_equal(C_r, oracle.centroids(X, want, K, sum_mode=1))


@pytest.mark.parametrize("K,cs", CODEBOOKS, ids=map(_id, CODEBOOKS))
def test_scattered_near_ties(engine, K, cs):
    """Pairs within 1e-17 ... 1e-3 relative whose two code vectors lie in different tiles and halves:
    the search's provisional index is often the wrong one of the two, far from the best in the tile
    order, and the recheck must still list both."""
    X, C, _ = rc.scattered_neartie(K, cs)
    want = oracle.kdtree_nn(C, X)
    engine.set_vectors(X)
    A = engine.assign(C)
    t = engine.timings()
    from helpers import neartie_cases as nt
    close = int(np.sum(nt.rel_gap(X, C) < 1e-9))
    print("flagged", t["flagged"][0], "rows within 1e-9:", close, "kd-tree rows", t["host_ties"][0])
    assert np.array_equal(A, want), "%d rows differ" % int(np.sum(A != want))
    assert close > 0 and t["flagged"][0] >= close
    C_r, A_r, _, info = engine.refine(K, C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1 and np.array_equal(A_r, want)
    assert np.array_equal(C_r, oracle.centroids(X, want, K, sum_mode=1))
